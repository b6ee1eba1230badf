"""A/B of the flat streaming kernel against copy_slices_kernel (run on MI355X).

HIPSTORE_FLAT / HIPSTORE_FLAT_SPAN / HIPSTORE_GRID / HIPSTORE_NT /
HIPSTORE_FLAT_NTLOAD are read per call, so one process sweeps every
combination.  Flat patterns, all through ``copy_batch``:

* ``one1g``   — a single 1 GiB copy;
* ``llama37`` — one Llama-3-8B-shaped state_dict sub-batch: 37 contiguous
  bf16 tensors (four decoder layers plus a slice of the embedding), ~2 GB,
  the size of one launch of the flagship bench;
* ``one2g``   — a single copy of llama37's total size, which separates the
  cost of many descriptors from the cost of the larger footprint.

Every configuration is timed REPEATS times (N calls each) and every repeat
is printed, so the repeat-to-repeat scatter is in the log next to the gain.

    python benchmarks/flat_copy_ab.py > profiles/flat_copy_ab.log
"""

import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from torchstore_amd.ops import gpu

REPEATS = 3
N = 10

KNOBS = ("HIPSTORE_FLAT", "HIPSTORE_FLAT_SPAN", "HIPSTORE_GRID",
         "HIPSTORE_NT", "HIPSTORE_FLAT_NTLOAD", "HIPSTORE_TILE")


def timeit(fn, n=N):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def llama_subbatch_numels():
    """37 entries: 4 decoder layers (9 tensors each) + 1/4 of the embedding."""
    h, kv, ffn, vocab = 4096, 1024, 14336, 128256
    layer = [h * h, kv * h, kv * h, h * h,      # wq wk wv wo
             ffn * h, h * ffn, ffn * h,          # w1 w2 w3
             h, h]                               # the two norms
    return layer * 4 + [vocab // 4 * h]


def main():
    torch.cuda.set_device(0)
    e = gpu.ext()
    dev = torch.device("cuda", 0)

    n1g = 1 << 30
    a1 = torch.empty(n1g, dtype=torch.uint8, device=dev)
    b1 = torch.empty(n1g, dtype=torch.uint8, device=dev)
    one1g = [(b1.data_ptr(), 0, a1.data_ptr(), 0, n1g)]

    numels = llama_subbatch_numels()
    srcs = [torch.empty(n, dtype=torch.bfloat16, device=dev) for n in numels]
    dsts = [torch.empty(n, dtype=torch.bfloat16, device=dev) for n in numels]
    llama37 = [(d.data_ptr(), 0, s.data_ptr(), 0, s.numel() * 2)
               for s, d in zip(srcs, dsts)]
    n2g = sum(numels) * 2
    a2 = torch.empty(n2g, dtype=torch.uint8, device=dev)
    b2 = torch.empty(n2g, dtype=torch.uint8, device=dev)
    one2g = [(b2.data_ptr(), 0, a2.data_ptr(), 0, n2g)]
    patterns = {
        "one1g": (one1g, 2 * n1g),
        "llama37": (llama37, 2 * n2g),
        "one2g": (one2g, 2 * n2g),
    }
    print(f"# one1g: 1 copy, {n1g} B; llama37: {len(llama37)} copies, "
          f"{n2g} B; one2g: 1 copy, {n2g} B; {REPEATS} repeats x {N} calls, "
          f"wall time per call incl. launch + sync")
    print(f"{'pattern':8s} {'flat':>4s} {'span':>7s} {'grid':>6s} {'nt':>2s} "
          f"{'ntl':>3s} " + " ".join(f"{'ms' + str(r):>7s}" for r in range(REPEATS))
          + f" {'GB/s med':>9s} {'scatter%':>8s}")

    results = []

    def run(name, flat, span, grid, nt, ntl):
        copies, moved = patterns[name]
        env = {"HIPSTORE_FLAT": flat, "HIPSTORE_GRID": grid,
               "HIPSTORE_NT": nt}
        if flat == "1":
            env["HIPSTORE_FLAT_SPAN"] = span
            env["HIPSTORE_FLAT_NTLOAD"] = ntl
        elif span != "-":
            env["HIPSTORE_TILE"] = span
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update({k: str(v) for k, v in env.items()})
        before = e.flat_launches()
        ts = sorted(timeit(lambda: e.copy_batch(copies))
                    for _ in range(REPEATS))
        used_flat = e.flat_launches() > before
        assert used_flat == (flat == "1"), "wrong kernel took the launch"
        med = ts[len(ts) // 2]
        bw = moved / med / 1e9
        scatter = (ts[-1] - ts[0]) / med * 100
        print(f"{name:8s} {flat:>4s} {span:>7s} {grid:>6s} {nt:>2s} "
              f"{ntl:>3s} " + " ".join(f"{t * 1e3:7.3f}" for t in ts)
              + f" {bw:9.1f} {scatter:8.2f}", flush=True)
        results.append((name, flat, span, grid, nt, ntl, bw))

    for name in patterns:
        # old kernel: its shipped default (tile by size, 8192 grid) and the
        # neighbouring settings of the earlier sweep
        for tile in ("-", "16384", "32768", "131072"):
            for grid in ("2048", "8192"):
                run(name, "0", tile, grid, "1", "-")
        # new kernel: span x grid, NT stores, plain and NT loads
        for ntl in ("0", "1"):
            for span in ("8192", "16384", "32768", "65536", "131072"):
                for grid in ("1024", "2048", "4096", "8192", "16384",
                             "65536"):
                    run(name, "1", span, grid, "1", ntl)
        # plain stores at the middle of the sweep
        for span in ("16384", "32768"):
            for grid in ("2048", "8192"):
                run(name, "1", span, grid, "0", "0")
    for k in KNOBS:
        os.environ.pop(k, None)

    print("\nbest per pattern and kernel (median GB/s, read+write):")
    for name in patterns:
        for flat in ("0", "1"):
            rows = [r for r in results if r[0] == name and r[1] == flat]
            b = max(rows, key=lambda r: r[6])
            print(f"  {name} flat={flat}: {b[6]:.1f} GB/s at span/tile={b[2]} "
                  f"grid={b[3]} nt={b[4]} ntload={b[5]}")


if __name__ == "__main__":
    main()
