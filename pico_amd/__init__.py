"""pico_amd -- libbine's reduce-family collectives (allreduce / reduce_scatter /
reduce) re-built for AMD MI355X: host-side Bine schedule planner, CDNA4 HIP
reduction kernels, RCCL point-to-point over xGMI.

The native library lives in pico_amd/lib/ (built in-tree by
``__graft_entry__.build()``); this package is a thin ctypes mirror of its C ABI
(include/bine_amd.h) with the reference's function names.

Element types: ``DTYPES`` are MPICH's 17 reduction types (the reference's);
``EXT_DTYPES`` adds "float16" and "bfloat16" (torch.float16 / torch.bfloat16),
reduced under sum / prod / max / min with every pairwise result correctly
rounded to the 16-bit format.

Scaled (averaging) forms: ``allreduce(..., scale=s)`` / ``reduce_scatter(...,
scale=s)`` return the unscaled call's bits times ``s`` (one multiplication per
element, defined in include/bine_amd.h), ``op="avg"`` is ``op="sum",
scale=1/comm.size``; floating types with sum / prod / max / min.  ``scale()``
is the arithmetic on its own.

Wide forms of the 16-bit types: ``allreduce_wide`` / ``reduce_scatter_wide``
(and ``reduce_tree_wide``, ``widen``, ``narrow``) reduce float16 / bfloat16
buffers with every pairwise operation in binary32 and ONE rounding to 16 bits
per output element: exactly the float32 call's result on the widened inputs,
rounded to nearest even.  ``wide_plan`` says which of the two bit-identical
paths a call takes.

Multi-buffer allreduce: ``allreduce_multi(algo, sbufs, rbufs, ...)`` reduces a
list of tensors as ONE collective -- the slices of the single call on their
concatenation, bit for bit (plain, ``scale=`` / ``op="avg"``, ``wide=True``).
``copy_segments`` is the many-ranges-one-launch device copy that packs and
unpacks them.

Sharded multi-buffer forms: ``reduce_scatter_multi`` leaves every rank its 1/P
shard of EACH tensor of a bucket, ``allgather_multi`` gathers a bucket of shards
back into the full tensors, each as ONE collective on the rank-major packing.
``copy_shards`` is the strided device copy (one descriptor per tensor) between
the two layouts.

Global norm and clipping: ``norm_multi`` gives every tensor's and the bucket's
squared L2 norm over all ranks (float64, deterministic bits), ``clip_multi``
then scales every tensor by min(1, max_norm / (norm + eps)) without a host
read.  ``sumsq_segments`` and ``clip_segments`` are the local halves: a
segmented sum of squares and a segmented scale whose factor is read from
device memory.

Optimizer step: ``adamw_segments`` is one fused AdamW update of a bucket of
shards (float32 p, m, v in place; the gradient read once, scaled by a device
coefficient; a 16-bit copy of the new parameter written where the allgather
wants it), bit for bit a float32 statement of one operation per line;
``adamw_multi`` adds the in-place ``allgather_multi`` of the full parameters.
``adamw_consts`` and ``plan_adamw`` are the host views of its constants and
launches.

Dynamic loss scaling: a 96-byte step state in device memory (``step_state_init``)
carries the loss scale and the step count.  ``step_update`` updates it on the
device from ``norm_multi``'s global squared norm -- infinite or NaN: skip and
back off; else the multiplier (clip / scale) and the step's constants --
and ``adamw_segments_dyn`` / ``adamw_multi_dyn`` take everything from it, storing
nothing on a skipped step: no host decision, no synchronization.
``step_update_host`` is the update's host twin, ``step_state_read`` the state as
a dict (it synchronizes).

MX-quantized gradient reduce-scatter: ``mx_reduce_scatter_multi`` quantizes
every shard of a bucket once to OCP MX blocks (32 elements per E8M0 scale byte,
e4m3 / e5m2 / e2m1 data), moves them in ONE all-to-all and leaves every rank
the float32-accumulated sum of its shards; ``mx_sum_segments`` is the receiving
half on its own (up to 16 wire blocks decoded and added in order),
``mx_wire_bytes`` and ``plan_mx_sum`` the host views of its layout and launches.
``mx_reduce_scatter_multi_ef`` is the same exchange with an error-feedback
residual: ``mx_quant_ef_segments`` quantizes gradient + residual in one pass and
stores what the format dropped back into the residual (float32, one per
element), so the error of a coordinate is sent with a later step, not lost;
``plan_mx_ef`` is the host view of its launches.
"""
from ._lib import ALGOS, DTYPES, EXT_DTYPES, OPS, BineError, lib  # noqa: F401
from .api import *  # noqa: F401,F403
from .api import __all__ as _api_all

__all__ = ["ALGOS", "DTYPES", "EXT_DTYPES", "OPS", "lib"] + _api_all
