"""Low-rank adapters (LoRA) on the linear projections of the encoder: query / key / value and the output projection of an attention
sub-layer, the up and down projections of a feed-forward sub-layer.

    from volta_amd.lora import add_lora, mark_only_lora_trainable
    add_lora(model, r=8, alpha=16, targets=("query", "value"), dropout=0.1)
    mark_only_lora_trainable(model, also=("clfs_dict.",))

An adapter is two ordinary parameters on the `LinearParams` holder of a projection, `lora_A` [r, in] and `lora_B` [out, r]; the engine adds
`(alpha / r) * (x A^T) B^T` to that projection's columns of the fused Q|K|V product with the kernels of csrc/lora.hip and returns both
parameters' gradients through the gradient arena, like any other weight's ("Low-rank adapters").  The targets
`attn_out` (attention_output.dense), `ffn_up` (intermediate.dense) and `ffn_down` (output.dense) run on the vk_lora_proj_* entry points:
the FFN-up adapter's term enters inside the GELU, the FFN-down adapter's input gradient passes through gelu'.  `dropout` is LoRA
dropout: in train mode the adapter (not the base projection) reads `keep * x / (1 - p)`, a Philox mask of its own per adapter and stream
made inside the kernels (vk_lora_*_drop) and replayed by the backward; eval mode and the retrieval scorer run without it.  One rank and
one rate per model; the e4m3 projection path refuses a model with adapters."""
import math

import torch
from torch import nn

from .modules import LinearParams, sublayer_schedule

TARGETS = ("query", "key", "value", "attn_out", "ffn_up", "ffn_down")
# target -> (kind of sub-layer that hosts it, module of the sub-layer, holder name of the text stream; the vision stream's is "v_" + that)
_PLACE = {"query": ("attn", "attention_self", "query"), "key": ("attn", "attention_self", "key"), "value": ("attn", "attention_self", "value"),
          "attn_out": ("attn", "attention_output", "dense"), "ffn_up": ("ff", "intermediate", "dense"), "ffn_down": ("ff", "output", "dense")}
RANKS = (4, 8, 16, 32)
_LEAVES = (".lora_A", ".lora_B")


def _root(model):
    return model.__dict__.get("_root") or model


def _encoder(root):
    return (root.bert if hasattr(root, "bert") else root).encoder


def _holders(root, targets=TARGETS, modalities=("text", "vision"), sublayers=None):
    """[(holder name relative to the root, holder)] in sub-layer order; within a sub-layer Q, K, V of the text stream, then of the vision
    stream, then the other targets of the text stream in the order of TARGETS, then those of the vision stream; a holder that serves both
    streams of a shared sub-layer is listed once."""
    enc = _encoder(root)
    prefix = "bert.encoder." if hasattr(root, "bert") else "encoder."
    out, seen = [], set()
    for k, (n, typ) in enumerate(sublayer_schedule(root.config)):
        if sublayers is not None and n not in sublayers:
            continue
        for group in (TARGETS[:3], TARGETS[3:]):
            for mod in ("text", "vision"):
                for t in group:
                    kind, module, base = _PLACE[t]
                    if kind != typ or t not in targets or mod not in modalities:
                        continue
                    node = enc.layer[k]._modules[module]
                    name = ("v_" if mod == "vision" else "") + base
                    holder = node._modules.get(name)
                    if isinstance(holder, LinearParams) and id(holder) not in seen:
                        seen.add(id(holder))
                        alias = base if node._modules.get(base) is holder else name          # a shared sub-layer's v_query IS query: its first name
                        out.append(("%slayer.%d.%s.%s" % (prefix, k, module, alias), holder))
    return out


def _adapted(root):
    return [(name, h) for name, h in _holders(root) if "lora_A" in h._parameters]


def _rate(dropout):
    p = float(dropout)
    if not 0.0 <= p < 1.0:          # NaN fails both comparisons
        raise ValueError("LoRA dropout %r: 0 <= p < 1" % (dropout,))
    return p


def add_lora(model, r=8, alpha=16, targets=("query", "value"), modalities=("text", "vision"), sublayers=None, seed=0, dropout=0.0):
    """Adds `lora_A` [r, in] (uniform in +-1 / sqrt(in), drawn on the CPU from torch.Generator().manual_seed(seed)) and `lora_B` [out, r]
    (zero) to every targeted projection; returns the new parameters' names.  Call it before the optimizer is built.  dropout: the rate of
    the dropout on the adapters' input in train mode (set_lora_dropout changes it later); `lora_config` lists it only when it is > 0."""
    root = _root(model)
    targets, modalities = tuple(targets), tuple(modalities)
    if r not in RANKS:
        raise ValueError("LoRA rank %r: one of %s" % (r, RANKS))
    if not targets or any(t not in TARGETS for t in targets) or len(set(targets)) != len(targets):
        raise ValueError("LoRA targets %r: a non-empty subset of %s" % (targets, TARGETS))
    if not modalities or any(m not in ("text", "vision") for m in modalities):
        raise ValueError("LoRA modalities %r: 'text' and / or 'vision'" % (modalities,))
    if not alpha > 0:
        raise ValueError("LoRA alpha %r must be positive" % (alpha,))
    p = _rate(dropout)
    if getattr(root, "lora_config", None) is not None or _adapted(root):
        raise RuntimeError("the model already has LoRA adapters (one rank and scale per model): merge_lora() or remove_lora() first")
    kinds = {_PLACE[t][0] for t in targets}
    hosts = [n for n, typ in sublayer_schedule(root.config) if typ in kinds]          # the sub-layers that host one of the chosen targets
    if sublayers is not None:
        sublayers = sorted(int(n) for n in sublayers)
        if not sublayers or any(n not in hosts for n in sublayers):
            raise ValueError("LoRA sublayers %r: the sub-layers of this config that host one of %r are %s" % (sublayers, targets, hosts))
    holders = _holders(root, targets, modalities, sublayers)
    if not holders:
        raise ValueError("no projection matches targets %r, modalities %r, sublayers %r" % (targets, modalities, sublayers))
    gen = torch.Generator().manual_seed(int(seed))
    names = []
    for name, h in holders:
        w = h.weight
        bound = 1.0 / math.sqrt(h.in_features)
        a = (torch.rand(r, h.in_features, generator=gen, dtype=torch.float32) * 2.0 - 1.0) * bound
        h.lora_A = nn.Parameter(a.to(w.device))
        h.lora_B = nn.Parameter(torch.zeros(h.out_features, r, dtype=torch.float32, device=w.device))
        for leaf in ("lora_A", "lora_B"):
            getattr(h, leaf)._vk_owner = root
            names.append("%s.%s" % (name, leaf))
    root.lora_config = dict(r=int(r), alpha=float(alpha), targets=list(targets), modalities=list(modalities),
                            sublayers=list(hosts if sublayers is None else sublayers))
    if p > 0.0:
        root.lora_config["dropout"] = p
    root._invalidate_engine()
    return names


def set_lora_dropout(model, p):
    """Changes the LoRA dropout rate of a model that has adapters (0 switches it off).  The cached plans go, the parameter arena stays."""
    root = _root(model)
    if getattr(root, "lora_config", None) is None:
        raise RuntimeError("the model has no LoRA adapters: add_lora() first")
    p = _rate(p)
    root.lora_config.pop("dropout", None)
    if p > 0.0:
        root.lora_config["dropout"] = p
    if root.__dict__.get("_engines"):
        root.__dict__["_engines"] = {}


def lora_dropout(model):
    cfg = getattr(_root(model), "lora_config", None)
    return 0.0 if cfg is None else cfg.get("dropout", 0.0)


def lora_scale(model):
    cfg = getattr(_root(model), "lora_config", None)
    return None if cfg is None else cfg["alpha"] / cfg["r"]


def mark_only_lora_trainable(model, also=()):
    """requires_grad False on everything but the adapters and the parameters whose names start with a prefix in `also`."""
    root = _root(model)
    if not _adapted(root):
        raise RuntimeError("the model has no LoRA adapters: add_lora() first")
    also = tuple(also)
    for n, p in root.named_parameters():
        p.requires_grad_(n.endswith(_LEAVES) or bool(also and n.startswith(also)))


def lora_state_dict(model):
    """The adapter entries of state_dict() (a shared sub-layer lists its adapter under both of its names, as it does its weights)."""
    return {k: v for k, v in _root(model).state_dict().items() if k.endswith(_LEAVES)}


def load_lora_state_dict(model, sd):
    """Strict on the adapter keys; touches nothing else."""
    root = _root(model)
    own = {k: v for k, v in root.state_dict(keep_vars=True).items() if k.endswith(_LEAVES)}
    missing, unexpected = sorted(set(own) - set(sd)), sorted(set(sd) - set(own))
    if missing or unexpected:
        raise KeyError("load_lora_state_dict: missing keys %s, unexpected keys %s" % (missing, unexpected))
    for k, p in own.items():
        if tuple(sd[k].shape) != tuple(p.shape):
            raise ValueError("load_lora_state_dict: %s has shape %s, the model's is %s" % (k, tuple(sd[k].shape), tuple(p.shape)))
    with torch.no_grad():
        for k, p in own.items():
            p.copy_(sd[k].to(device=p.device, dtype=p.dtype))


def _drop(root, merge):
    holders = _adapted(root)
    if not holders:
        raise RuntimeError("the model has no LoRA adapters")
    s = lora_scale(root)
    with torch.no_grad():
        for _, h in holders:
            if merge:
                h.weight.add_(h.lora_B.detach().float() @ h.lora_A.detach().float(), alpha=s)
            del h._parameters["lora_A"], h._parameters["lora_B"]
    root.lora_config = None
    root._invalidate_engine()


def merge_lora(model):
    """W += (alpha / r) * B @ A in fp32 on the master weights, then the adapters go: state_dict() has the reference's keys again."""
    _drop(_root(model), True)


def remove_lora(model):
    """Drops the adapters without merging."""
    _drop(_root(model), False)
