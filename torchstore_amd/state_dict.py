"""state_dict exchange: flatten → batched put, with a commit marker.

Reference semantics (torchstore ``state_dict_utils.py``):

* ``put_state_dict`` flattens the nested dict (torch DCP's util), optionally
  casts floating tensors to a transfer dtype, batch-puts every entry under
  ``"{key}/{flat_key}"`` and writes ``"{key}/<MAPPING>"`` **last** — readers
  fetch the mapping first, so a partially-pushed state_dict is invisible
  (the commit-marker protocol);
* ``get_state_dict`` fetches the mapping (missing ⇒ "no matching push"),
  batch-gets all entries (in place into the user's state_dict tensors when
  given — DTensor entries reshard per-entry), and unflattens.

On GPU the dtype cast uses the fused cast+pack HIP kernel (K3) so the
staging copy and the cast are one kernel pass.

``transfer_quant`` ships and stores selected entries as block-scaled FP8
(``ops/quant.py``): the payload travels under the entry's usual key, its
scales under ``"{key}/<FP8_SCALES>/{flat_key}"``, and the commit marker —
a :class:`QuantMapping` — records which flat keys are quantised and their
original dtype, so readers learn it from the fetch they already make.
``transfer_quant="mxfp4"`` does the same with MXFP4 (``ops/mx.py``): scales
under ``"{key}/<MX_SCALES>/{flat_key}"``, and the marker's ``mx`` field
records the original dtype and the logical shape (an odd last dimension
cannot be told from the packed payload).  A push uses one policy.
"""

from __future__ import annotations

import asyncio
import fnmatch
import os
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import torch

from torchstore_amd.client import LocalClient
from torchstore_amd.ops.mx import (
    MxQuantizedTensor,
    alloc_mx,
    dequantize_mxfp4_into,
    mx_shapes,
    quantize_mxfp4,
)
from torchstore_amd.ops.quant import (
    QUANT_DTYPES,
    QuantizedTensor,
    alloc_quantized,
    dequantize_fp8_into,
    quantize_fp8,
    scales_shape,
)
from torchstore_amd.utils.logging import LatencyTracker, get_logger

logger = get_logger("torchstore_amd.state_dict")

MAPPING_KEY = "<MAPPING>"
# scales of quantised entries live under this reserved segment, next to
# <MAPPING>: a flat key never starts with an angle-bracket segment of ours
SCALES_KEY = "<FP8_SCALES>"
MX_SCALES_KEY = "<MX_SCALES>"
_SCALES_KEYS = (SCALES_KEY, MX_SCALES_KEY)


def _selects(policy, flat_key: str, value: Any) -> bool:
    return (
        type(value) is torch.Tensor
        and value.dtype in QUANT_DTYPES
        and value.dim() >= 1
        and value.numel() >= policy.min_numel
        and not any(fnmatch.fnmatchcase(flat_key, p) for p in policy.exclude)
    )


@dataclass(frozen=True)
class Fp8BlockQuant:
    """``transfer_quant`` policy: block-scaled FP8 e4m3, blocks of 128.

    A state_dict entry is quantised when it is a plain ``torch.Tensor`` (no
    subclass, so DTensor entries are left alone) of dtype f32/bf16/f16 with
    at least one dimension and ``min_numel`` elements, whose flat key matches
    none of the ``exclude`` fnmatch patterns.
    """

    min_numel: int = 0
    exclude: Sequence[str] = ()

    def selects(self, flat_key: str, value: Any) -> bool:
        return _selects(self, flat_key, value)


@dataclass(frozen=True)
class Mxfp4BlockQuant:
    """``transfer_quant`` policy: MXFP4, packed e2m1 values with one e8m0
    scale byte per block of 32 (``ops/mx.py``).  Selects entries by the same
    rule as :class:`Fp8BlockQuant`."""

    min_numel: int = 0
    exclude: Sequence[str] = ()

    def selects(self, flat_key: str, value: Any) -> bool:
        return _selects(self, flat_key, value)


TransferQuant = Union[None, str, Fp8BlockQuant, Mxfp4BlockQuant]


def _resolve_quant(
    transfer_quant: TransferQuant,
) -> Union[None, Fp8BlockQuant, Mxfp4BlockQuant]:
    if transfer_quant is None or isinstance(
        transfer_quant, (Fp8BlockQuant, Mxfp4BlockQuant)
    ):
        return transfer_quant
    if transfer_quant == "fp8_e4m3":
        return Fp8BlockQuant()
    if transfer_quant == "mxfp4":
        return Mxfp4BlockQuant()
    raise ValueError(
        f"unknown transfer_quant {transfer_quant!r}: expected 'fp8_e4m3', "
        "'mxfp4', an Fp8BlockQuant or an Mxfp4BlockQuant"
    )


class QuantMapping(dict):
    """The commit marker of a quantised push: the usual flat-key mapping plus
    ``quant``, ``{flat_key: original dtype}`` of the FP8 entries, or ``mx``,
    ``{flat_key: (original dtype, logical shape)}`` of the MXFP4 ones.  A
    plain push keeps writing a plain dict, so readers tell them apart from
    the marker they fetch anyway."""

    def __init__(
        self,
        mapping=(),
        quant: Optional[Dict[str, torch.dtype]] = None,
        mx: Optional[Dict[str, Tuple[torch.dtype, Tuple[int, ...]]]] = None,
    ):
        super().__init__(mapping)
        self.quant = dict(quant or {})
        self.mx = dict(mx or {})

    def __reduce__(self):
        # without MXFP4 entries the marker pickles as it did before they
        # existed: plain and FP8 pushes stay byte-identical on the wire
        if not self.mx:
            return (QuantMapping, (dict(self), self.quant))
        return (QuantMapping, (dict(self), self.quant, self.mx))

# pipeline factor: big state_dicts move as N concurrent sub-batches so RPC
# framing/parsing overlaps the volume's bulk copies
_PIPELINE = max(1, int(os.environ.get("TORCHSTORE_AMD_SD_PIPELINE", "8")))


async def _get_pipeline(client: LocalClient) -> int:
    """Gets already fan out one RPC per involved volume; extra client-side
    splitting only multiplies per-RPC launch/sync overhead once the volume
    count itself provides the concurrency."""
    volumes = await client._ensure_volumes()
    return max(1, _PIPELINE // max(1, len(volumes)))


def _split(d: Dict[str, Any], n: int) -> List[Dict[str, Any]]:
    if n <= 1 or len(d) <= 8:
        return [d]
    items = list(d.items())
    size = (len(items) + n - 1) // n
    return [dict(items[i : i + size]) for i in range(0, len(items), size)]


def _flatten(state_dict: Dict[str, Any]):
    from torch.distributed.checkpoint._nested_dict import flatten_state_dict

    return flatten_state_dict(state_dict)


def _unflatten(flat: Dict[str, Any], mapping):
    from torch.distributed.checkpoint._nested_dict import unflatten_state_dict

    return unflatten_state_dict(flat, mapping)


def _cast_floating(
    flat: Dict[str, Any], dtype: Optional[torch.dtype]
) -> Dict[str, Any]:
    if dtype is None:
        return flat
    from torchstore_amd.ops.cast import cast_tensor

    out = {}
    for k, v in flat.items():
        if isinstance(v, torch.Tensor) and v.is_floating_point():
            out[k] = cast_tensor(v, dtype)
        else:
            out[k] = v
    return out


def _nbytes(flat: Dict[str, Any]) -> int:
    total = 0
    for v in flat.values():
        if isinstance(v, torch.Tensor):
            total += v.numel() * v.element_size()
    return total


def _scales_beside_payloads(
    fetches: Dict[str, Any], key: str, flat_keys
) -> Dict[str, Any]:
    """Order ``fetches`` so every scales entry follows its payload: ``_split``
    cuts by entry count, and scales trailing at the end would leave all the
    bytes in the first sub-batches."""
    out: Dict[str, Any] = {}
    for k in flat_keys:
        out[f"{key}/{k}"] = fetches[f"{key}/{k}"]
        for scales_key in _SCALES_KEYS:
            sk = f"{key}/{scales_key}/{k}"
            if sk in fetches:
                out[sk] = fetches[sk]
    return out


def _plan_quant_dests(
    key: str,
    user_flat: Dict[str, Any],
    quant: Dict[str, torch.dtype],
    fetches: Dict[str, Any],
) -> List[Tuple[Tuple[torch.Tensor, torch.Tensor], torch.Tensor]]:
    """Point the fetches of quantised entries at FP8 destinations.

    A ``QuantizedTensor`` leaf receives payload and scales in place.  A
    tensor leaf gets scratch buffers on its own device; the returned
    ``[((payload, scales), dest), ...]`` is what remains to dequantise once
    the fetches have landed.
    """
    wanted = [k for k in user_flat if k in quant]
    if not wanted:
        return []
    by_device: Dict[torch.device, List[str]] = {}
    for k in wanted:
        leaf = user_flat[k]
        if isinstance(leaf, QuantizedTensor):
            if tuple(leaf.scales.shape) != scales_shape(leaf.payload.shape):
                raise ValueError(
                    f"QuantizedTensor destination for {k!r}: scales shape "
                    f"{tuple(leaf.scales.shape)} does not belong to a payload "
                    f"of shape {tuple(leaf.payload.shape)}"
                )
            fetches[f"{key}/{k}"] = leaf.payload
            fetches[f"{key}/{SCALES_KEY}/{k}"] = leaf.scales
        elif (
            type(leaf) is torch.Tensor
            and leaf.dtype in QUANT_DTYPES
            and leaf.dim() >= 1
        ):
            by_device.setdefault(leaf.device, []).append(k)
        else:
            raise TypeError(
                f"entry {k!r} was pushed quantised: its destination must be "
                "a plain f32/bf16/f16 tensor or a QuantizedTensor, got "
                f"{type(leaf).__name__}"
            )
    pending = []
    for device, ks in by_device.items():
        bufs = alloc_quantized([user_flat[k].shape for k in ks], device)
        for k, (payload, scales) in zip(ks, bufs):
            fetches[f"{key}/{k}"] = payload
            fetches[f"{key}/{SCALES_KEY}/{k}"] = scales
            pending.append(((payload, scales), user_flat[k]))
    return pending


def _plan_mx_dests(
    key: str,
    user_flat: Dict[str, Any],
    mx: Dict[str, Tuple[torch.dtype, Tuple[int, ...]]],
    fetches: Dict[str, Any],
) -> List[Tuple[Tuple[torch.Tensor, torch.Tensor], torch.Tensor]]:
    """``_plan_quant_dests`` for MXFP4 entries: an ``MxQuantizedTensor`` leaf
    receives payload and scales in place, a tensor leaf gets scratch buffers
    and is dequantised into afterwards.  Either must have the logical shape
    the marker recorded."""
    by_device: Dict[torch.device, List[str]] = {}
    for k in user_flat:
        if k not in mx:
            continue
        leaf = user_flat[k]
        shape = tuple(mx[k][1])
        if isinstance(leaf, MxQuantizedTensor):
            got = (tuple(leaf.payload.shape), tuple(leaf.scales.shape))
            if tuple(leaf.shape) != shape or got != mx_shapes(shape):
                raise ValueError(
                    f"MxQuantizedTensor destination for {k!r}: shape "
                    f"{tuple(leaf.shape)} with payload/scales {got} does "
                    f"not fit the stored entry of shape {shape}"
                )
            fetches[f"{key}/{k}"] = leaf.payload
            fetches[f"{key}/{MX_SCALES_KEY}/{k}"] = leaf.scales
        elif (
            type(leaf) is torch.Tensor
            and leaf.dtype in QUANT_DTYPES
            and leaf.dim() >= 1
        ):
            if tuple(leaf.shape) != shape:
                raise ValueError(
                    f"destination for {k!r} has shape {tuple(leaf.shape)}, "
                    f"the stored MXFP4 entry {shape}"
                )
            by_device.setdefault(leaf.device, []).append(k)
        else:
            raise TypeError(
                f"entry {k!r} was pushed quantised: its destination must be "
                "a plain f32/bf16/f16 tensor or an MxQuantizedTensor, got "
                f"{type(leaf).__name__}"
            )
    pending = []
    for device, ks in by_device.items():
        bufs = alloc_mx([user_flat[k].shape for k in ks], device)
        for k, (payload, scales) in zip(ks, bufs):
            fetches[f"{key}/{k}"] = payload
            fetches[f"{key}/{MX_SCALES_KEY}/{k}"] = scales
            pending.append(((payload, scales), user_flat[k]))
    return pending


# per-(client, key) direct-sync endpoints, built lazily on first use
_direct_sources: Dict[tuple, Any] = {}
_direct_dests: Dict[tuple, Any] = {}


async def put_state_dict(
    client: LocalClient,
    state_dict: Dict[str, Any],
    key: str,
    transfer_dtype: Optional[torch.dtype] = None,
    direct: bool = False,
    rank: Optional[int] = None,
    world_size: Optional[int] = None,
    direct_rdma: bool = False,  # reference-compat alias for ``direct``
    transfer_quant: TransferQuant = None,
) -> None:
    direct = direct or direct_rdma
    quant = _resolve_quant(transfer_quant)
    if direct and quant is not None:
        raise ValueError(
            "transfer_quant is not supported with direct=True: quantised "
            "direct sync needs shard-aware scale geometry (docs/ROADMAP.md)"
        )
    if direct:
        from torchstore_amd.weight_sync import DirectWeightSyncSource

        ck = (id(client), key)
        source = _direct_sources.get(ck)
        if source is None:
            source = DirectWeightSyncSource(
                client, key, transfer_dtype, rank=rank, world_size=world_size
            )
            _direct_sources[ck] = source
        await source.push(state_dict)
        return
    tracker = LatencyTracker(f"put_state_dict[{key}]")
    flat, mapping = _flatten(state_dict)
    tracker.step("flatten")
    if quant is not None:
        # the whole dict in one kernel launch, before the split into
        # sub-batches; the other floating entries still take transfer_dtype
        qkeys = [k for k, v in flat.items() if quant.selects(k, v)]
        if isinstance(quant, Mxfp4BlockQuant):
            scales_key = MX_SCALES_KEY
            pairs = dict(zip(qkeys, quantize_mxfp4([flat[k] for k in qkeys])))
            mapping = QuantMapping(
                mapping,
                mx={k: (flat[k].dtype, tuple(flat[k].shape)) for k in qkeys},
            )
        else:
            scales_key = SCALES_KEY
            pairs = dict(zip(qkeys, quantize_fp8([flat[k] for k in qkeys])))
            mapping = QuantMapping(mapping, {k: flat[k].dtype for k in qkeys})
        rest = _cast_floating(
            {k: v for k, v in flat.items() if k not in pairs}, transfer_dtype
        )
        # scales ride next to their payload, so the sub-batches of the
        # pipeline stay balanced in bytes
        staged: Dict[str, Any] = {}
        for k in flat:
            if k in pairs:
                staged[k], staged[f"{scales_key}/{k}"] = pairs[k]
            else:
                staged[k] = rest[k]
        flat = staged
        tracker.step("quant+cast")
    else:
        flat = _cast_floating(flat, transfer_dtype)
        tracker.step("cast")
    prefixed = {f"{key}/{k}": v for k, v in flat.items()}
    await asyncio.gather(
        *(client.put_batch(chunk) for chunk in _split(prefixed, _PIPELINE))
    )
    tracker.step("put_batch", _nbytes(flat))
    # commit marker: written last, fetched first by readers
    await client.put(f"{key}/{MAPPING_KEY}", mapping)
    tracker.step("commit")
    tracker.e2e(_nbytes(flat))


async def get_state_dict(
    client: LocalClient,
    key: str,
    user_state_dict: Optional[Dict[str, Any]] = None,
    strict: bool = True,
    direct: bool = False,
    direct_rdma: bool = False,  # reference-compat alias for ``direct``
    dequantize: bool = True,
) -> Dict[str, Any]:
    """``dequantize`` matters only for entries pushed with ``transfer_quant``
    and only when no ``user_state_dict`` is given: ``False`` returns them as
    :class:`QuantizedTensor` (FP8) or :class:`MxQuantizedTensor` (MXFP4)
    leaves instead of tensors of the original dtype.  With a
    ``user_state_dict`` the destination leaf decides: a tensor (f32/bf16/f16)
    is dequantised into, a ``QuantizedTensor`` / ``MxQuantizedTensor``
    receives payload and scales as stored."""
    direct = direct or direct_rdma
    if direct:
        from torchstore_amd.weight_sync import DirectWeightSyncDest

        if user_state_dict is None:
            raise ValueError("direct get_state_dict needs a destination state_dict")
        ck = (id(client), key)
        dest = _direct_dests.get(ck)
        if dest is None:
            dest = DirectWeightSyncDest(client, key)
            _direct_dests[ck] = dest
        await dest.pull(user_state_dict)
        return user_state_dict
    tracker = LatencyTracker(f"get_state_dict[{key}]")
    try:
        mapping = await client.get(f"{key}/{MAPPING_KEY}")
    except KeyError as exc:
        raise RuntimeError(
            f"no state_dict was pushed under {key!r} (missing commit marker)"
        ) from exc
    tracker.step("mapping")
    # {flat_key: original dtype} of the quantised entries; empty for a
    # plain push, and then everything below is what it always was
    quant: Dict[str, torch.dtype] = getattr(mapping, "quant", {})
    # {flat_key: (original dtype, logical shape)} of the MXFP4 entries
    mx: Dict[str, Tuple[torch.dtype, Tuple[int, ...]]] = getattr(
        mapping, "mx", {}
    )

    if user_state_dict is not None:
        user_flat, user_mapping = _flatten(user_state_dict)
        if strict:
            # reference asserts MAPPING EQUALITY, both directions
            # (torchstore state_dict_utils.py:146-152): entries the user
            # has but the store doesn't AND entries the store has but the
            # user doesn't are both strict-mode errors
            stored_keys = {str(k) for k in mapping}
            missing = set(user_flat.keys()) - stored_keys
            extra = stored_keys - set(user_flat.keys())
            if missing or extra:
                raise KeyError(
                    f"strict get_state_dict mapping mismatch: "
                    f"user-only entries {sorted(missing)[:5]}, "
                    f"stored-only entries {sorted(extra)[:5]}"
                )
        fetches = {f"{key}/{k}": v for k, v in user_flat.items()}
        pending = _plan_quant_dests(key, user_flat, quant, fetches)
        mx_pending = _plan_mx_dests(key, user_flat, mx, fetches)
        if quant or mx:
            fetches = _scales_beside_payloads(fetches, key, user_flat)
        chunks = await asyncio.gather(
            *(
                client.get_batch(c)
                for c in _split(fetches, await _get_pipeline(client))
            )
        )
        results = {}
        for c in chunks:
            results.update(c)
        tracker.step("get_batch", _nbytes(user_flat))
        flat = {
            k: user_flat[k]
            if k in quant or k in mx
            else results[f"{key}/{k}"]
            for k in user_flat
        }
        if pending:
            # one batched dequant lands in the user's tensors in place
            dequantize_fp8_into(
                [pair for pair, _ in pending], [dst for _, dst in pending]
            )
            tracker.step("dequant")
        if mx_pending:
            dequantize_mxfp4_into(
                [pair for pair, _ in mx_pending],
                [dst for _, dst in mx_pending],
            )
            tracker.step("dequant")
        out = _unflatten(flat, user_mapping)
        tracker.e2e(_nbytes(user_flat))
        return out

    flat_keys = list(mapping.keys())
    fetches = {f"{key}/{k}": None for k in flat_keys}
    if quant:
        fetches.update({f"{key}/{SCALES_KEY}/{k}": None for k in quant})
        fetches = _scales_beside_payloads(fetches, key, flat_keys)
    if mx:
        fetches.update({f"{key}/{MX_SCALES_KEY}/{k}": None for k in mx})
        fetches = _scales_beside_payloads(fetches, key, flat_keys)
    chunks = await asyncio.gather(
        *(
            client.get_batch(c)
            for c in _split(fetches, await _get_pipeline(client))
        )
    )
    results = {}
    for c in chunks:
        results.update(c)
    tracker.step("get_batch")
    flat = {k: results[f"{key}/{k}"] for k in flat_keys}
    if quant:
        leaves = {
            k: QuantizedTensor(
                flat[k], results[f"{key}/{SCALES_KEY}/{k}"], dtype
            )
            for k, dtype in quant.items()
        }
        if dequantize:
            outs = [
                torch.empty(q.shape, dtype=q.orig_dtype, device=q.payload.device)
                for q in leaves.values()
            ]
            dequantize_fp8_into(
                [(q.payload, q.scales) for q in leaves.values()], outs
            )
            flat.update(zip(leaves.keys(), outs))
            tracker.step("dequant")
        else:
            flat.update(leaves)
    if mx:
        mx_leaves = {
            k: MxQuantizedTensor(
                flat[k], results[f"{key}/{MX_SCALES_KEY}/{k}"], shape, dtype
            )
            for k, (dtype, shape) in mx.items()
        }
        if dequantize:
            outs = [
                torch.empty(q.shape, dtype=q.orig_dtype, device=q.payload.device)
                for q in mx_leaves.values()
            ]
            dequantize_mxfp4_into(
                [(q.payload, q.scales) for q in mx_leaves.values()], outs
            )
            flat.update(zip(mx_leaves.keys(), outs))
            tracker.step("dequant")
        else:
            flat.update(mx_leaves)
    out = _unflatten(flat, mapping)
    tracker.e2e(_nbytes(flat))
    return out
