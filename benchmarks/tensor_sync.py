"""Per-tensor FP8 sync: kernel rates and end-to-end effect (run on MI355X).

(a) Kernel rates: quantise and dequantise 1 GiB of bf16 as one large matrix,
    as a stack of 256 small matrices (a fused MoE weight) and as a Llama-like
    mix of 19 tensors in one batch.  GB/s counts one read and one write of
    every element plus the scales, the bytes of the block-scaled FP8 kernels
    (K4/K5), which run on the same data in the same run as the yardstick.
    The per-tensor quantise (K14) is two launches and reads the source TWICE,
    so by bytes moved (5 against 3 per bf16 element) it should land near 3/5
    of K4's rate; the dequantise (K15) moves K5's bytes.  HIPSTORE_TENSOR_GRID
    is read per call, so one process also times other grid caps: every shape
    has about 32768 quantise units, so a cap of 65536 is one workgroup and
    one atomic per unit, and a lower cap means several units per workgroup
    and one atomic per workgroup and matrix that it meets.  The defaults are
    8192 for the quantise and 65536 for the dequantise.
(b) End to end: the Llama-3-8B-shaped dict of ``bench.py`` on one GPU,
    ``put_state_dict`` + ``get_state_dict`` into bf16 destinations, plain,
    block-scaled and per-tensor, and the bytes each push leaves resident.

Every configuration is timed REPEATS times and every repeat is printed, so
the repeat-to-repeat scatter stands next to the medians.  A repeat is N calls
after WARM warm-up calls (about 0.1 s of kernel time); the four kernels at
the defaults, whose ratios are reported, take their repeats in turn.

    python benchmarks/tensor_sync.py > profiles/tensor_sync.log
"""

import asyncio
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from torchstore_amd.ops import gpu
from torchstore_amd.ops.quant import scales_shape
from torchstore_amd.ops.quant_tensor import tensor_scales_shape

REPEATS = 3
N = 300
WARM = 10
STEPS = 5
WARMUP = 2
_LAYER = [(4096, 4096), (1024, 4096), (1024, 4096), (4096, 4096),
          (14336, 4096), (14336, 4096), (4096, 14336), (4096,), (4096,)]
# 512 Mi elements each
SHAPES = {
    "131072 x 4096": [(131072, 4096)],
    "256 x 1024 x 2048": [(256, 1024, 2048)],
    "Llama-like mix (2 layers + 24572 x 4096)": _LAYER * 2 + [(24572, 4096)],
}
KNOB = "HIPSTORE_TENSOR_GRID"


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


def kernel_rates():
    dev = torch.device("cuda", 0)
    print(f"# (a) kernel rates; {REPEATS} repeats x {N} calls after {WARM} "
          "warm-up calls, wall time per call incl. launch + sync; GB/s = one "
          "read + one write of every element, plus scales")
    for label, shapes in SHAPES.items():
        def bufs(dtype, shape_of=lambda s: s):
            return [torch.empty(shape_of(s), dtype=dtype, device=dev) for s in shapes]

        xs = bufs(torch.bfloat16)
        for x in xs:
            x.normal_(0, 0.02)
        ys, payloads = bufs(torch.bfloat16), bufs(torch.float8_e4m3fn)
        bscales = bufs(torch.float32, scales_shape)
        tscales = bufs(torch.float32, tensor_scales_shape)
        numel = sum(x.numel() for x in xs)
        bbytes = numel * 3 + sum(s.numel() for s in bscales) * 4
        tbytes = numel * 3 + sum(s.numel() for s in tscales) * 4
        units = sum(s.numel() * -(-(x.numel() // s.numel()) // 16384)
                    for x, s in zip(xs, tscales))
        print(f"\n## {label}: {len(xs)} tensors, {numel} bf16 elements, "
              f"{sum(s.numel() for s in tscales)} matrices, {units} quantise units")
        print(f"{'kernel':22s} {'knob':>12s} "
              + " ".join(f"{'ms' + str(r):>7s}" for r in range(REPEATS))
              + f" {'GB/s med':>9s} {'scatter%':>8s}")
        os.environ.pop(KNOB, None)
        dflt = [
            ("quant_fp8 (block)", bbytes,
             lambda: gpu.quant_fp8_batch(list(zip(xs, payloads, bscales)), dev)),
            ("dequant_fp8 (block)", bbytes,
             lambda: gpu.dequant_fp8_batch(list(zip(ys, payloads, bscales)), dev)),
            ("quant_tensor", tbytes,
             lambda: gpu.quant_tensor_batch(list(zip(xs, payloads, tscales)), dev)),
            ("dequant_tensor", tbytes,
             lambda: gpu.dequant_tensor_batch(list(zip(ys, payloads, tscales)), dev)),
        ]
        # the compared kernels in turn, so a drift of the machine hits all four
        times = [[timeit(fn) for _, _, fn in dflt] for _ in range(REPEATS)]
        bq, bd, q, d = (
            row(name, "dflt", moved, None, [t[i] for t in times])
            for i, (name, moved, _) in enumerate(dflt)
        )
        print(f"ratio to the block kernels at the defaults: quant {q / bq:.2f}, "
              f"dequant {d / bd:.2f}")
        for g in (2048, 8192, 65536):
            os.environ[KNOB] = str(g)
            row("quant_tensor", f"grid={g}", tbytes, dflt[2][2])
            row("dequant_tensor", f"grid={g}", tbytes, dflt[3][2])
        os.environ.pop(KNOB, None)
        del xs, ys, payloads, bscales, tscales, dflt
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
    print(f"{'mode':16s} {'put ms':>24s} {'get ms':>24s} {'put+get med':>12s} "
          f"{'resident GB':>12s}")
    try:
        resident_before = 0
        for mode in ("plain", "fp8_e4m3", "fp8_e4m3_tensor"):
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
            print(f"{mode:16s} "
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
