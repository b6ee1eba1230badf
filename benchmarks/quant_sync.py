"""Block-scaled FP8 sync: kernel rates and end-to-end effect (run on MI355X).

(a) Kernel rates: quantise and dequantise 1 GiB of bf16 (2^29 elements),
    read + write bytes per second, beside ``cast_copy`` bf16->f16 at the same
    numel in the same run — the existing memory-bound kernel is the
    yardstick.  HIPSTORE_QUANT_GRID is read per call, so one process sweeps
    the grid cap.
(b) End to end: the Llama-3-8B-shaped dict of ``bench.py`` on one GPU,
    ``put_state_dict`` + ``get_state_dict`` into bf16 destinations, with and
    without ``transfer_quant``, and the bytes each push leaves resident in
    the volume.

Every configuration is timed REPEATS times and every repeat is printed, so
the repeat-to-repeat scatter stands next to the medians.

    python benchmarks/quant_sync.py > profiles/quant_sync.log
"""

import asyncio
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from torchstore_amd.ops import gpu

REPEATS = 3
N = 10
STEPS = 5
WARMUP = 2


def timeit(fn, n=N):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def row(name, grid, moved, fn):
    ts = sorted(timeit(fn) for _ in range(REPEATS))
    med = ts[len(ts) // 2]
    print(f"{name:22s} {grid:>6s} "
          + " ".join(f"{t * 1e3:7.3f}" for t in ts)
          + f" {moved / med / 1e9:9.1f} {(ts[-1] - ts[0]) / med * 100:8.2f}",
          flush=True)
    return moved / med / 1e9


def kernel_rates():
    dev = torch.device("cuda", 0)
    rows, cols = 32768, 16384  # 2^29 elements, 1 GiB of bf16
    numel = rows * cols
    x = torch.empty(rows, cols, dtype=torch.bfloat16, device=dev).normal_(0, 0.02)
    payload = torch.empty(rows, cols, dtype=torch.float8_e4m3fn, device=dev)
    scales = torch.empty(rows, cols // 128, dtype=torch.float32, device=dev)
    y = torch.empty(rows, cols, dtype=torch.bfloat16, device=dev)
    h = torch.empty(rows, cols, dtype=torch.float16, device=dev)
    qbytes = numel * 2 + numel + scales.numel() * 4
    print(f"# (a) kernel rates, {numel} elements; {REPEATS} repeats x {N} "
          "calls, wall time per call incl. launch + sync; GB/s = read + write")
    print(f"{'kernel':22s} {'grid':>6s} "
          + " ".join(f"{'ms' + str(r):>7s}" for r in range(REPEATS))
          + f" {'GB/s med':>9s} {'scatter%':>8s}")
    os.environ.pop("HIPSTORE_QUANT_GRID", None)
    row("cast_copy bf16->f16", "dflt", numel * 4, lambda: gpu.cast_copy(x, h))
    best = {}
    for grid in ("dflt", "256", "512", "1024", "2048", "4096", "8192", "16384",
                 "65536"):
        if grid == "dflt":
            os.environ.pop("HIPSTORE_QUANT_GRID", None)
        else:
            os.environ["HIPSTORE_QUANT_GRID"] = grid
        q = row("quant_fp8 bf16", grid, qbytes,
                lambda: gpu.quant_fp8_batch([(x, payload, scales)], dev))
        d = row("dequant_fp8 ->bf16", grid, qbytes,
                lambda: gpu.dequant_fp8_batch([(y, payload, scales)], dev))
        if grid != "dflt":
            best[grid] = (q, d)
    os.environ.pop("HIPSTORE_QUANT_GRID", None)
    gq = max(best, key=lambda g: best[g][0])
    gd = max(best, key=lambda g: best[g][1])
    print(f"best grid cap: quant {gq} ({best[gq][0]:.1f} GB/s), "
          f"dequant {gd} ({best[gd][1]:.1f} GB/s)")
    del x, payload, scales, y, h
    torch.cuda.empty_cache()


async def end_to_end():
    import torchstore_amd as ts
    from torchstore_amd.models import llama
    from torchstore_amd.strategy import LocalRankStrategy

    src = llama.make_local_shard_state_dict(
        0, 1, llama.fsdp_placement, device="cuda:0", pattern=True
    )
    dst = llama.make_local_shard_state_dict(
        0, 1, llama.tp_placement, device="cuda:0"
    )
    payload = llama.total_bytes(llama.llama3_8b_shapes(), torch.bfloat16)
    await ts.initialize(
        num_storage_volumes=1, strategy=LocalRankStrategy(),
        storage_device="auto",
    )
    print(f"\n# (b) end to end, Llama-3-8B shapes, {len(src)} entries, "
          f"{payload / 1e9:.2f} GB bf16, 1 GPU; {WARMUP} warm-up + {STEPS} "
          f"steps per repeat, {REPEATS} repeats; ms per step, median of "
          "repeats last")
    print(f"{'mode':10s} {'put ms':>24s} {'get ms':>24s} {'put+get med':>12s} "
          f"{'resident GB':>12s}")
    try:
        resident_before = 0
        for mode, kw in (("plain", {}), ("fp8_e4m3", {"transfer_quant": "fp8_e4m3"})):
            key = f"bench_{mode}"
            puts, gets = [], []
            for _ in range(REPEATS):
                tp = tg = 0.0
                for step in range(WARMUP + STEPS):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    await ts.put_state_dict(src, key, **kw)
                    t1 = time.perf_counter()
                    await ts.get_state_dict(key, dst)
                    torch.cuda.synchronize()
                    t2 = time.perf_counter()
                    if step >= WARMUP:
                        tp += t1 - t0
                        tg += t2 - t1
                puts.append(tp / STEPS * 1e3)
                gets.append(tg / STEPS * 1e3)
            stats = await ts.stats()
            resident = sum(v["tensor_bytes"] for v in stats["volumes"])
            both = sorted(p + g for p, g in zip(puts, gets))
            print(f"{mode:10s} "
                  + f"{' '.join(f'{p:7.2f}' for p in puts):>24s} "
                  + f"{' '.join(f'{g:7.2f}' for g in gets):>24s} "
                  + f"{both[len(both) // 2]:12.2f} "
                  + f"{(resident - resident_before) / 1e9:12.2f}",
                  flush=True)
            resident_before = resident
    finally:
        await ts.shutdown()


def main():
    torch.cuda.set_device(0)
    gpu.ext()
    kernel_rates()
    asyncio.run(end_to_end())


if __name__ == "__main__":
    main()
