"""MXFP4 sync: kernel rates and end-to-end effect (run on MI355X).

(a) Kernel rates: quantise and dequantise 1 GiB of bf16 (2^29 elements) as
    MXFP4, read + write bytes per second, beside the FP8 kernels and
    ``cast_copy`` bf16->f16 at the same numel in the same run.  The kernels
    are memory-bound, so bytes moved per second is the figure to compare.
    HIPSTORE_MX_GRID is read per call, so one process sweeps the grid cap.
(b) End to end: the Llama-3-8B-shaped dict of ``bench.py`` on one GPU,
    ``put_state_dict`` + ``get_state_dict`` into bf16 destinations, plain,
    FP8 and MXFP4, and the bytes each push leaves resident in the volume.

Every configuration is timed REPEATS times and every repeat is printed.

    python benchmarks/mx_sync.py > profiles/mx_sync.log
    python benchmarks/mx_sync.py --kernels-only     # part (a) alone
"""

import asyncio
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from benchmarks.quant_sync import REPEATS, STEPS, WARMUP, N, row
from torchstore_amd.ops import gpu

GRIDS = ("dflt", "256", "1024", "2048", "4096", "8192", "16384", "32768",
         "65536", "262144")


def kernel_rates():
    dev = torch.device("cuda", 0)
    rows, cols = 32768, 16384  # 2^29 elements, 1 GiB of bf16
    numel = rows * cols
    x = torch.empty(rows, cols, dtype=torch.bfloat16, device=dev).normal_(0, 0.02)
    y = torch.empty(rows, cols, dtype=torch.bfloat16, device=dev)
    h = torch.empty(rows, cols, dtype=torch.float16, device=dev)
    p8 = torch.empty(rows, cols, dtype=torch.float8_e4m3fn, device=dev)
    s8 = torch.empty(rows, cols // 128, dtype=torch.float32, device=dev)
    p4 = torch.empty(rows, cols // 2, dtype=torch.uint8, device=dev)
    s4 = torch.empty(rows, cols // 32, dtype=torch.uint8, device=dev)
    bytes8 = numel * 2 + numel + s8.numel() * 4
    bytes4 = numel * 2 + p4.numel() + s4.numel()
    print(f"# (a) kernel rates, {numel} elements, {gpu.ext().MX_LANES} "
          f"lane(s) per MXFP4 block; {REPEATS} repeats x {N} calls, wall time "
          "per call incl. launch + sync; GB/s = read + write")
    print(f"{'kernel':22s} {'grid':>6s} "
          + " ".join(f"{'ms' + str(r):>7s}" for r in range(REPEATS))
          + f" {'GB/s med':>9s} {'scatter%':>8s}")
    for knob in ("HIPSTORE_QUANT_GRID", "HIPSTORE_MX_GRID"):
        os.environ.pop(knob, None)
    row("cast_copy bf16->f16", "dflt", numel * 4, lambda: gpu.cast_copy(x, h))
    row("quant_fp8 bf16", "dflt", bytes8,
        lambda: gpu.quant_fp8_batch([(x, p8, s8)], dev))
    row("dequant_fp8 ->bf16", "dflt", bytes8,
        lambda: gpu.dequant_fp8_batch([(y, p8, s8)], dev))
    best = {}
    for grid in GRIDS:
        if grid == "dflt":
            os.environ.pop("HIPSTORE_MX_GRID", None)
        else:
            os.environ["HIPSTORE_MX_GRID"] = grid
        q = row("quant_mx bf16", grid, bytes4,
                lambda: gpu.quant_mx_batch([(x, p4, s4)], dev))
        d = row("dequant_mx ->bf16", grid, bytes4,
                lambda: gpu.dequant_mx_batch([(y, p4, s4)], dev))
        if grid != "dflt":
            best[grid] = (q, d)
    os.environ.pop("HIPSTORE_MX_GRID", None)
    gq = max(best, key=lambda g: best[g][0])
    gd = max(best, key=lambda g: best[g][1])
    print(f"best grid cap: quant {gq} ({best[gq][0]:.1f} GB/s), "
          f"dequant {gd} ({best[gd][1]:.1f} GB/s)")
    del x, y, h, p8, s8, p4, s4
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
        for mode in (None, "fp8_e4m3", "mxfp4"):
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
    torch.cuda.set_device(0)
    gpu.ext()
    kernel_rates()
    if "--kernels-only" not in sys.argv:
        asyncio.run(end_to_end())


if __name__ == "__main__":
    main()
