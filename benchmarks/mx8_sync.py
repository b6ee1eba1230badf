"""MXFP8 sync: kernel rates against K4/K5 and end-to-end effect (run on MI355X).

(a) Kernel rates: quantise and dequantise 1 GiB of bf16 (2^29 elements, one
    matrix) as MXFP8, read + write bytes per second.  The yardstick is the
    block-scaled FP8 pair K4/K5, which moves the same bytes per element
    (3 + 1/32 against 3 + 4/128): it is timed before the sweep of
    HIPSTORE_MX8_GRID, in the middle of it and after it, so its own
    run-to-run spread stands next to the ratio.  The knob is read per call,
    so one process sweeps the grid cap.  The conversion form and the
    scale-store variant are compile-time choices of csrc/quant_mx8.h: run
    the script once per build and name the build with ``--label``.
(b) End to end: the Llama-3-8B-shaped dict of ``bench.py`` on one GPU,
    ``put_state_dict`` + ``get_state_dict`` into bf16 destinations, plain,
    FP8 and MXFP8, and the bytes each push leaves resident.

Every configuration is timed REPEATS times and every repeat is printed.

    python benchmarks/mx8_sync.py --label "..." > profiles/mx8_sync.log
    python benchmarks/mx8_sync.py --kernels-only --label "..."   # (a) alone
"""

import asyncio
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from benchmarks.quant_sync import REPEATS, STEPS, WARMUP, N, row
from torchstore_amd.ops import gpu

GRIDS = ("dflt", "1024", "4096", "16384", "65536", "262144")


def kernel_rates(label):
    dev = torch.device("cuda", 0)
    rows, cols = 32768, 16384  # 2^29 elements, 1 GiB of bf16
    numel = rows * cols
    x = torch.empty(rows, cols, dtype=torch.bfloat16, device=dev).normal_(0, 0.02)
    y = torch.empty(rows, cols, dtype=torch.bfloat16, device=dev)
    p8 = torch.empty(rows, cols, dtype=torch.float8_e4m3fn, device=dev)
    s8 = torch.empty(rows, cols // 128, dtype=torch.float32, device=dev)
    pm = torch.empty(rows, cols, dtype=torch.float8_e4m3fn, device=dev)
    sm = torch.empty(rows, cols // 32, dtype=torch.uint8, device=dev)
    bytes8 = numel * 3 + s8.numel() * 4
    bytesm = numel * 3 + sm.numel()
    print(f"# (a) kernel rates, {numel} elements, build: {label}; {REPEATS} "
          f"repeats x {N} calls, wall time per call incl. launch + sync; "
          "GB/s = read + write")
    print(f"{'kernel':22s} {'grid':>6s} "
          + " ".join(f"{'ms' + str(r):>7s}" for r in range(REPEATS))
          + f" {'GB/s med':>9s} {'scatter%':>8s}")
    for knob in ("HIPSTORE_QUANT_GRID", "HIPSTORE_MX8_GRID"):
        os.environ.pop(knob, None)
    fp8 = []

    def fp8_rows():
        fp8.append((
            row("quant_fp8 bf16", "dflt", bytes8,
                lambda: gpu.quant_fp8_batch([(x, p8, s8)], dev)),
            row("dequant_fp8 ->bf16", "dflt", bytes8,
                lambda: gpu.dequant_fp8_batch([(y, p8, s8)], dev)),
        ))

    best = {}
    fp8_rows()
    for i, grid in enumerate(GRIDS):
        if grid == "dflt":
            os.environ.pop("HIPSTORE_MX8_GRID", None)
        else:
            os.environ["HIPSTORE_MX8_GRID"] = grid
        best[grid] = (
            row("quant_mx8 bf16", grid, bytesm,
                lambda: gpu.quant_mx8_batch([(x, pm, sm)], dev)),
            row("dequant_mx8 ->bf16", grid, bytesm,
                lambda: gpu.dequant_mx8_batch([(y, pm, sm)], dev)),
        )
        if i in (0, len(GRIDS) // 2):
            fp8_rows()
    os.environ.pop("HIPSTORE_MX8_GRID", None)
    fp8_rows()
    dflt = best.pop("dflt")
    gq = max(best, key=lambda g: best[g][0])
    gd = max(best, key=lambda g: best[g][1])
    print(f"best grid cap: quant {gq} ({best[gq][0]:.1f} GB/s), "
          f"dequant {gd} ({best[gd][1]:.1f} GB/s)")
    for side, name in ((0, "quant"), (1, "dequant")):
        rates = sorted(r[side] for r in fp8)
        med = rates[len(rates) // 2]
        print(f"{name}: mx8 (default grid) / fp8 (median of {len(rates)} "
              f"runs) = {dflt[side] / med:.3f}; fp8 run-to-run spread "
              f"{(rates[-1] - rates[0]) / med * 100:.2f}%")
    del x, y, p8, s8, pm, sm
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
        for mode in (None, "fp8_e4m3", "mxfp8_e4m3"):
            key = f"bench_{mode or 'plain'}"
            puts, gets = [], []
            for _ in range(REPEATS):
                tp = tg = 0.0
                for step in range(WARMUP + STEPS):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    await ts.put_state_dict(src, key, transfer_quant=mode)
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
            print(f"{mode or 'plain':10s} "
                  + f"{' '.join(f'{p:7.2f}' for p in puts):>24s} "
                  + f"{' '.join(f'{g:7.2f}' for g in gets):>24s} "
                  + f"{both[len(both) // 2]:12.2f} "
                  + f"{(resident - resident_before) / 1e9:12.2f}",
                  flush=True)
            resident_before = resident
    finally:
        await ts.shutdown()


def main():
    label = "as built"
    if "--label" in sys.argv:
        label = sys.argv[sys.argv.index("--label") + 1]
    torch.cuda.set_device(0)
    gpu.ext()
    kernel_rates(label)
    if "--kernels-only" not in sys.argv:
        asyncio.run(end_to_end())


if __name__ == "__main__":
    main()
