"""Host side of the MI355X engine: flat parameter arenas and the static execution plan.

Design: for a given (batch, text length, region count) every activation, weight and gradient
buffer is fixed, so a pre-training step is compiled ONCE into two command lists (forward, backward) of
pre-bound kernel launches (`vk_op`, include/volta_hip.h) that the C++ executor replays each step.  No
autograd graph, no per-op Python: `BertForVLPreTraining.forward` costs one C call, `backward` another.

Parameters live in one flat fp32 arena (each nn.Parameter is a view of it), mirrored by a bf16 shadow
arena (MFMA operands), a fp32 gradient arena (wgrad GEMMs write straight into it; DDP buckets are ranges
of it) and, in the optimizer, two moment arenas.  Q/K/V weights of a sub-layer are adjacent, so the three
projections run as one [3H, H] GEMM.

Dropout sites are numbered in the order of the reference's forward (embeddings; per sub-layer: tt, tv,
vv, vt probabilities, text output, vision output; pooled) -- the contract the mask-replay tests rely on.
"""
from .arena import CHUNK, NO_DECAY, ParamArena
from .builder import StepEngine, Stream, pair_segments, wide_geometry, canonical_frozen, frozen_blocks
from .heads import VIS_TARGET_WIDTH
from .plan import Plan
