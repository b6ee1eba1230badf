"""Row-scaled FP8 sync: kernel rates and end-to-end effect (run on MI355X).

(a) Kernel rates: quantise and dequantise 1 GiB of bf16 in three shapes, one
    per regime of K10 (wave per row, workgroup holding the row, workgroup
    streaming it), read + write bytes per second.  The block-scaled FP8
    kernels (K4/K5) run on the same data in the same run as the yardstick:
    the same bytes plus 3 % more scales.  HIPSTORE_ROW_GRID is read per call,
    so one process sweeps the grid cap; HIPSTORE_ROW_WAVE / HIPSTORE_ROW_WG
    lower the regime limits, so each shape is also timed in the next regime
    up (what a smaller W or R would make of it).
(b) End to end: the Llama-3-8B-shaped dict of ``bench.py`` on one GPU,
    ``put_state_dict`` + ``get_state_dict`` into bf16 destinations, plain,
    block-scaled and row-scaled, and the bytes each push leaves resident.

Every configuration is timed REPEATS times and every repeat is printed, so
the repeat-to-repeat scatter stands next to the medians.  A repeat is N calls
after WARM warm-up calls (about 0.1 s of kernel time); the four kernels at
the defaults, whose ratios are reported, take their repeats in turn.  The
three shapes have at most 65536 units, fewer than the grid cap, so (c) sweeps
the cap on 2 GiB of 1024-wide rows: 262144 quantise and 131072 dequantise
units.

    python benchmarks/row_sync.py > profiles/row_sync.log
"""

import asyncio
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from torchstore_amd.ops import gpu

REPEATS = 3
N = 300
WARM = 10
STEPS = 5
WARMUP = 2
SHAPES = [(131072, 4096), (37449, 14336), (8192, 65536)]
KNOBS = ("HIPSTORE_ROW_GRID", "HIPSTORE_ROW_WAVE", "HIPSTORE_ROW_WG")


def timeit(fn, n=N):
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def row(name, knob, moved, fn, ts=None):
    ts = sorted(ts or [timeit(fn) for _ in range(REPEATS)])
    med = ts[len(ts) // 2]
    print(f"{name:22s} {knob:>12s} "
          + " ".join(f"{t * 1e3:7.3f}" for t in ts)
          + f" {moved / med / 1e9:9.1f} {(ts[-1] - ts[0]) / med * 100:8.2f}",
          flush=True)
    return moved / med / 1e9


def set_knobs(**kw):
    for k in KNOBS:
        os.environ.pop(k, None)
    for k, v in kw.items():
        os.environ[f"HIPSTORE_ROW_{k}"] = str(v)


def kernel_rates():
    dev = torch.device("cuda", 0)
    W, R = gpu.row_limits()
    print(f"# (a) kernel rates, compiled limits W={W} R={R}; {REPEATS} repeats "
          f"x {N} calls after {WARM} warm-up calls, wall time per call incl. "
          "launch + sync; GB/s = read + write")
    for rows, cols in SHAPES:
        numel = rows * cols
        x = torch.empty(rows, cols, dtype=torch.bfloat16, device=dev).normal_(0, 0.02)
        payload = torch.empty(rows, cols, dtype=torch.float8_e4m3fn, device=dev)
        bscales = torch.empty(rows, cols // 128, dtype=torch.float32, device=dev)
        rscales = torch.empty(rows, 1, dtype=torch.float32, device=dev)
        y = torch.empty(rows, cols, dtype=torch.bfloat16, device=dev)
        bbytes = numel * 3 + bscales.numel() * 4
        rbytes = numel * 3 + rows * 4
        regime = "wave" if cols <= W else "held" if cols <= R else "stream"
        print(f"\n## {rows} x {cols} bf16, regime {regime}")
        print(f"{'kernel':22s} {'knob':>12s} "
              + " ".join(f"{'ms' + str(r):>7s}" for r in range(REPEATS))
              + f" {'GB/s med':>9s} {'scatter%':>8s}")
        set_knobs()
        dflt = [
            ("quant_fp8 (block)", bbytes,
             lambda: gpu.quant_fp8_batch([(x, payload, bscales)], dev)),
            ("dequant_fp8 (block)", bbytes,
             lambda: gpu.dequant_fp8_batch([(y, payload, bscales)], dev)),
            ("quant_row", rbytes,
             lambda: gpu.quant_row_batch([(x, payload, rscales)], dev)),
            ("dequant_row", rbytes,
             lambda: gpu.dequant_row_batch([(y, payload, rscales)], dev)),
        ]
        # the compared kernels in turn, so a drift of the machine hits all four
        times = [[timeit(fn) for _, _, fn in dflt] for _ in range(REPEATS)]
        bq, bd, q, d = (
            row(name, "dflt", moved, None, [t[i] for t in times])
            for i, (name, moved, _) in enumerate(dflt)
        )
        print(f"ratio to the block kernels at the defaults: quant {q / bq:.2f}, "
              f"dequant {d / bd:.2f}")
        configs = [(f"grid={g}", {"GRID": g})
                   for g in (1024, 4096, 16384, 65536)]
        if regime == "wave":
            configs += [("W=1024", {"WAVE": 1024})]  # held by the workgroup
        if regime != "stream":
            configs += [("W=R=1024", {"WAVE": 1024, "WG": 1024})]  # streamed
        for label, kw in configs:
            set_knobs(**kw)
            row("quant_row", label, rbytes, dflt[2][2])
            if "W" not in label:  # the limits do not touch the dequant side
                row("dequant_row", label, rbytes, dflt[3][2])
        set_knobs()
        del x, payload, bscales, rscales, y
        torch.cuda.empty_cache()


def grid_cap():
    dev = torch.device("cuda", 0)
    rows, cols = 1048576, 1024
    x = torch.empty(rows, cols, dtype=torch.bfloat16, device=dev).normal_(0, 0.02)
    payload = torch.empty(rows, cols, dtype=torch.float8_e4m3fn, device=dev)
    scales = torch.empty(rows, 1, dtype=torch.float32, device=dev)
    moved = rows * cols * 3 + rows * 4
    print(f"\n# (c) grid cap above and below the unit count: {rows} x {cols} "
          "bf16 (2 GiB), 262144 quantise and 131072 dequantise units")
    print(f"{'kernel':22s} {'knob':>12s} "
          + " ".join(f"{'ms' + str(r):>7s}" for r in range(REPEATS))
          + f" {'GB/s med':>9s} {'scatter%':>8s}")
    for g in (16384, 65536, 131072, 262144):
        set_knobs(GRID=g)
        row("quant_row", f"grid={g}", moved,
            lambda: gpu.quant_row_batch([(x, payload, scales)], dev))
        row("dequant_row", f"grid={g}", moved,
            lambda: gpu.dequant_row_batch([(x, payload, scales)], dev))
    set_knobs()


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
    print(f"{'mode':14s} {'put ms':>24s} {'get ms':>24s} {'put+get med':>12s} "
          f"{'resident GB':>12s}")
    try:
        resident_before = 0
        for mode in ("plain", "fp8_e4m3", "fp8_e4m3_row"):
            kw = {} if mode == "plain" else {"transfer_quant": mode}
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
            print(f"{mode:14s} "
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
    grid_cap()
    asyncio.run(end_to_end())


if __name__ == "__main__":
    main()
