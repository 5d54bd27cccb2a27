"""Drop-in model classes: same constructor / forward signatures, parameter names and error behaviour as the
reference's `BertModel` / `BertForVLPreTraining` (volta/encoders.py:918-1114, volta/utils.py:250-360), with the
whole forward + backward dispatched to the HIP engine (volta_amd/engine/).  There is no eager / CPU
fallback: without a GPU and libvolta_hip.so the forward raises.

Differences a caller can observe, all deliberate:
  * the three losses come back from one fused step; the two host synchronisations of the reference
    (encoders.py:1089, 1111) do not happen -- `img_loss` is numerically 0 when no region is labelled;
  * activations are bf16 with fp32 accumulation / statistics (north_star), parameters stay fp32;
  * dropout uses a counter-based Philox stream seeded from `torch.initial_seed()` (or `set_dropout_seed`).
"""
import logging
import os
import weakref

import torch
from torch import nn

from . import modules as M
from .config import BertConfig

logger = logging.getLogger(__name__)


class ArenaParameters:
    """What `parameters()` of a volta_amd root model returns: nn.Module's parameter iterator, carrying the model it walks.
    `clip_grad_norm_(model.parameters(), max_norm)` -- the reference's call, train_concap.py:307 -- reads `vk_model` and takes the whole
    gradient arena in one pass instead of walking 600 tensors (an explicit hook: no generator-frame introspection)."""

    __slots__ = ("vk_model", "started", "_it")

    def __init__(self, model, it):
        self.vk_model, self.started, self._it = model, False, it

    def __iter__(self):
        return self

    def __next__(self):
        self.started = True
        return next(self._it)


class PreTrainedModel(nn.Module):
    """Base with the helpers the reference's driver touches (volta/utils.py:250-360)."""

    def parameters(self, recurse=True):
        it = super().parameters(recurse)
        return ArenaParameters(self, it) if (recurse and getattr(self, "_vk_is_model", False)) else it

    config_class = BertConfig
    base_model_prefix = "bert"
    _arena_prefix = ""

    def __init__(self, config, *inputs, **kwargs):
        super().__init__()
        self.config = config

    def init_weights(self, module):
        M.init_bert_(module, self.config.initializer_range)

    def _get_resized_embeddings(self, old_embeddings, new_num_tokens=None):
        if new_num_tokens is None:
            return old_embeddings
        old_num_tokens, dim = old_embeddings.weight.size()
        if old_num_tokens == new_num_tokens:
            return old_embeddings
        new = M.TableParams(new_num_tokens, dim).to(old_embeddings.weight.device)
        new.weight.data.normal_(mean=0.0, std=self.config.initializer_range)
        n = min(old_num_tokens, new_num_tokens)
        new.weight.data[:n, :] = old_embeddings.weight.data[:n, :]
        self._invalidate_engine()
        return new

    def _tie_or_clone_weights(self, first_module, second_module):
        first_module.weight = second_module.weight

    def _invalidate_engine(self):
        root = getattr(self, "_root", None) or self
        root.__dict__["_arena"] = None
        root.__dict__["_engines"] = {}

    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)       # .cuda() / .to() / .float(): parameters are re-allocated
        self._invalidate_engine()
        return out

    def save_pretrained(self, save_directory):
        assert os.path.isdir(save_directory), "Saving path should be a directory where the model and configuration can be saved"
        model_to_save = self.module if hasattr(self, "module") else self
        with open(os.path.join(save_directory, "config.json"), "w", encoding="utf-8") as f:
            f.write(model_to_save.config.to_json_string())
        torch.save({k: v.detach().cpu().clone() for k, v in model_to_save.state_dict().items()},
                   os.path.join(save_directory, "pytorch_model.bin"))

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, *model_args, config=None, state_dict=None, **kwargs):
        """Local directory / file branch of the reference loader (volta/utils.py:404-550): old `gamma` / `beta` names,
        the HuggingFace-BERT key renumbering of `from_hf=True` (`bert_layer2attn_sublayer` / `bert_layer2ff_sublayer`,
        utils.py:475-498), base-model checkpoints without the `bert.` prefix (utils.py:513-521), tied decoder, eval mode,
        `output_loading_info`.  Named archives would need the network (utils.py:417-418) and are refused."""
        kwargs.pop("default_gpu", None)
        kwargs.pop("cache_dir", None)
        from_hf = kwargs.pop("from_hf", False)
        output_loading_info = kwargs.pop("output_loading_info", False)
        if kwargs.pop("from_tf", False):
            raise NotImplementedError("TensorFlow checkpoints (volta/utils.py:424-426) are not supported")
        assert config is not None
        path = pretrained_model_name_or_path
        if path is not None and os.path.isdir(path):
            path = os.path.join(path, "pytorch_model.bin")
        if state_dict is None:
            if path is None or not os.path.isfile(path):
                raise EnvironmentError("'%s' is not a local checkpoint; downloading named archives is not available "
                                       "offline (volta/utils.py:417-418)" % pretrained_model_name_or_path)
            state_dict = torch.load(path, map_location="cpu")
        model = cls(config, *model_args, **kwargs)
        sd = {}
        for k, v in state_dict.items():                       # old LayerNorm parameter names (utils.py:461-472)
            if "gamma" in k:
                k = k.replace("gamma", "weight")
            if "beta" in k:
                k = k.replace("beta", "bias")
            sd[k[len("module."):] if k.startswith("module.") else k] = v     # (DDP-wrapped saves; train_utils.py:326-330)
        if from_hf:                                           # one BERT layer -> one attention + one FF sub-layer
            a2s, f2s = config.bert_layer2attn_sublayer, config.bert_layer2ff_sublayer
            renames = []
            for k in sd:
                if ".layer." not in k:
                    continue
                num = int(k.split(".layer.")[-1].split(".")[0])
                nk = None
                if ".attention." in k:
                    nk = k.replace(".layer.%d.attention." % num, ".layer.%d.attention_" % a2s.get(str(num), num))
                elif ".intermediate." in k:
                    nk = k.replace(".layer.%d.intermediate." % num, ".layer.%d.intermediate." % f2s.get(str(num), num))
                elif ".output." in k:
                    nk = k.replace(".layer.%d.output." % num, ".layer.%d.output." % f2s.get(str(num), num))
                if nk:
                    renames.append((k, nk, num))
            for k, nk, _ in sorted(renames, key=lambda x: x[2], reverse=True):      # highest layer first: no clobbering
                sd[nk] = sd.pop(k)
        # derived model <- base checkpoint, or base model <- derived checkpoint (utils.py:511-521)
        prefix = cls.base_model_prefix + "."
        has_prefix = any(k.startswith(prefix) for k in sd)
        target, rel = model, ""
        if hasattr(model, cls.base_model_prefix) and not has_prefix:
            target = getattr(model, cls.base_model_prefix)
        elif not hasattr(model, cls.base_model_prefix) and has_prefix:
            rel = prefix
        if rel:
            sd = {k[len(rel):]: v for k, v in sd.items() if k.startswith(rel)}
        res = target.load_state_dict(sd, strict=False)
        missing, unexpected = list(res.missing_keys), list(res.unexpected_keys)
        if missing:
            print("Weights of {} not initialized from pretrained model: {}".format(cls.__name__, missing))
        if unexpected:
            print("Weights from pretrained model not used in {}: {}".format(cls.__name__, unexpected))
        if hasattr(model, "tie_weights"):
            model.tie_weights()
        model.eval()
        if output_loading_info:
            return model, {"missing_keys": missing, "unexpected_keys": unexpected, "error_msgs": []}
        return model


class BertEncoder(M.Holder):
    def __init__(self, config):
        super().__init__()
        self.num2type = {}
        layers = []
        for n, typ in M.sublayer_schedule(config):
            self.num2type[n] = typ
            layers.append(M.build_attention_sublayer(config, n) if typ == "attn" else M.build_ffn_sublayer(config, n))
        self.layer = nn.ModuleList(layers)


class EngineHostModel(PreTrainedModel):
    """What BertModel, BertForVLPreTraining and BertForVLTasks share as root models: the state of a root model (`_ROOT_STATE`), the flat
    parameter arena, the cache of engine plans and the host side of one engine step.  The model that holds another one takes its
    parameters and its root state (`_adopt`); the nested model keeps `_root` only."""

    _heads_mode = "pretrain"           # StepEngine(heads=...)
    _torch_param_prefixes = ()         # parameters of torch-side head modules: autograd, not the engine, writes their gradients
    task_cfg = None
    lora_config = None                 # volta_amd.lora.add_lora: dict(r, alpha, targets, modalities, sublayers[, dropout]) while the model has adapters
    # `_vk_is_model` lets clip_grad_norm_(model.parameters()) recognise the whole arena without walking it: on the instance, a nested model is none
    _ROOT_STATE = dict(_vk_is_model=True, _arena=None, _engines=None, _step=0, _seed_base=None, _last=None, _ddp=None, _fwd_serial=0,
                       _fp8=False, _task_dropout=0.1)

    def _init_root_state(self, task_dropout=0.1):
        """Last step of a root model's constructor.  `_root` and `_ddp` are modules: in `__dict__`, out of nn.Module's registration."""
        self.add_global_imgfeat = int(self.config.add_global_imgfeat is not None)
        self.__dict__.update(self._ROOT_STATE, _engines={}, _task_dropout=float(task_dropout))
        for mod in self.modules():
            if mod is not self and isinstance(mod, EngineHostModel):
                mod._adopt(self)
        for p in self.parameters():            # lets an optimizer find (and materialize) its model before the first forward,
            p._vk_owner = self                 # e.g. AdamW.load_state_dict() in the reference's resume() order

    def _adopt(self, root):
        """Called by the root model that holds this one: the parameters become the root's, the standalone state goes."""
        self.__dict__["_root"] = root
        for k in self._ROOT_STATE:
            self.__dict__.pop(k, None)

    def set_dropout_seed(self, seed):
        self._seed_base, self._step = int(seed), 0

    def set_projection_dtype(self, dtype):
        """"bf16" (default) or "fp8": run the forward Q|K|V / FFN projections of the encoder on the e4m3 MFMA path (csrc/fp8.hip)."""
        if dtype not in ("bf16", "fp8"):
            raise ValueError("projection dtype %r (bf16 | fp8)" % (dtype,))
        self._fp8 = dtype == "fp8"

    def materialize(self, device=None):
        """Build (or rebuild) the flat parameter arenas on `device`; parameters become views of them.  (Nested: the root model's.)"""
        root = self.__dict__.get("_root")
        if root is not None:
            return root.materialize(device)
        from .engine import ParamArena
        dev = torch.device(device) if device is not None else next(self.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("volta_amd runs on an MI355X only: move the model to the GPU first (model.cuda()); "
                               "there is no CPU execution path")
        arena = self._arena
        if arena is None or arena.device != dev or not arena.intact():
            self._arena, self._engines = ParamArena(self, dev, prefix=self._arena_prefix), {}
            for p in self.parameters():
                p._vk_owner = self
        return self._arena

    def _frozen_signature(self, arena):
        """The pruning decision of the parameters' current requires_grad pattern (engine.canonical_frozen): a frozenset of arena names,
        empty when no block is frozen as a whole.  One pass over the parameters per forward; the decision of the last pattern is kept."""
        pattern = tuple(p.requires_grad for _, p in arena.param_list())
        memo = arena.frozen_memo
        if memo is None or memo[0] != pattern:
            sig = frozenset()
            if not all(pattern):
                from .engine import canonical_frozen
                sig = canonical_frozen(arena, [n for (n, _), on in zip(arena.param_list(), pattern) if not on], self._heads_mode)
            memo = arena.frozen_memo = (pattern, sig)
        return memo[1]

    def _engine(self, B, T, Rv, train, task_id=None, maps=False):
        from .engine import StepEngine
        arena = self.materialize()
        key = (B, T, Rv, bool(train), self._fp8, task_id, maps)
        # frozen parameters (requires_grad False) prune the backward list: the plan is keyed by what they prune, and by nothing more
        # when they prune nothing -- flipping requires_grad between steps selects (or builds) the matching plan
        frozen = self._frozen_signature(arena)
        if frozen:
            key += (frozen,)
        eng = self._engines.get(key)
        if eng is None:
            for k in [k for k in self._engines if k[3] == key[3] and k[5] == task_id and k[6] == maps]:      # one plan per mode (and task head) keeps memory bounded
                del self._engines[k]
            task = (task_id, self.task_cfg[task_id]) if task_id is not None else None
            eng = StepEngine(self.config, arena, B, T, Rv, train, heads=self._heads_mode, fp8=self._fp8, task=task,
                             task_dropout=self._task_dropout, attn_maps=maps, frozen=frozen, lora_dropout=(self.lora_config or {}).get("dropout", 0.0))
            self._engines[key] = eng
        return eng

    def _prep_inputs(self, input_ids, image_feat, image_loc, token_type_ids, attention_mask, image_attention_mask,
                     masked_lm_labels=None, image_label=None, image_cls=None, next_sentence_label=None, obj_labels=None, obj_confs=None,
                     attr_labels=None, attr_confs=None):
        dev = next(self.parameters()).device
        B, T = input_ids.shape
        Rv = image_feat.shape[1]
        i64 = dict(device=dev, dtype=torch.int64)
        f32 = dict(device=dev, dtype=torch.float32)
        if attention_mask is None:
            attention_mask = torch.ones(B, T, **i64)
        if token_type_ids is None:
            token_type_ids = torch.zeros(B, T, **i64)
        if image_attention_mask is None:
            image_attention_mask = torch.ones(B, Rv, **i64)
        R = Rv - self.add_global_imgfeat
        t = dict(input_ids=input_ids.to(**i64).contiguous(), token_type_ids=token_type_ids.to(**i64).contiguous(),
                 attention_mask=attention_mask.to(**i64).contiguous(), image_attention_mask=image_attention_mask.to(**i64).contiguous(),
                 image_feat=image_feat.to(**f32).contiguous(), image_loc=image_loc.to(**f32).contiguous())
        assert t["image_feat"].shape == (B, Rv, self.config.v_feature_size), "image_feat must be [B, regions, v_feature_size]"
        assert t["image_loc"].shape == (B, Rv, self.config.num_locs), "image_loc must be [B, regions, num_locs]"
        if masked_lm_labels is not None:
            t["masked_lm_labels"] = masked_lm_labels.to(**i64).contiguous()
            t["image_label"] = image_label.to(**i64).contiguous()
            assert t["masked_lm_labels"].shape == (B, T) and t["image_label"].shape == (B, R)
            # what each configured visual target reads (volta/losses.py); the reference silently drops a target whose inputs are
            # missing -- here that is an error, the plan was compiled for the configured targets
            need = set()
            for ix, w in self.config.visual_target_weights.items():
                if w > 0:
                    need |= {"0": {"image_cls"}, "3": {"obj_labels", "obj_confs"}, "4": {"attr_labels", "attr_confs"}, "6": {"obj_labels"}}.get(ix, set())
            given = dict(image_cls=image_cls, obj_labels=obj_labels, obj_confs=obj_confs, attr_labels=attr_labels, attr_confs=attr_confs)
            for name in sorted(need):
                if given[name] is None:
                    raise ValueError("visual target weights %r need `%s`" % (self.config.visual_target_weights, name))
                x = given[name].to(**(i64 if name.endswith("labels") else f32)).contiguous()
                assert x.shape[:2] == (B, R), "%s must be [B, regions%s]" % (name, ", 1601" if name == "image_cls" else "")
                t[name] = x
            if "image_cls" in t:
                assert t["image_cls"].shape == (B, R, 1601)
            if self.config.fusion_method in ("mul", "sum", "text"):
                if next_sentence_label is None:
                    raise ValueError("fusion method %r has an ITM head: next_sentence_label is required" % self.config.fusion_method)
                t["next_sentence_label"] = next_sentence_label.to(**i64).contiguous()
                assert t["next_sentence_label"].numel() == B
            # ids / labels are range-clamped inside the kernels: no host synchronisation on the hot path
        return t, B, T, Rv

    def _engine_forward(self, tensors, task_id=None, attn_maps=False):
        """One forward list: the plan of this shape and mode, with `task_id`'s classifier behind the poolers and, with `attn_maps`, every
        attention sub-layer's probabilities kept.  Returns the pre-training losses (None on the other plans)."""
        B, T = tensors["input_ids"].shape
        Rv = tensors["image_feat"].shape[1]
        eng = self._engine(B, T, Rv, self.training, task_id, bool(attn_maps))
        eng.arena.refresh_shadow()
        if eng.fp8:
            eng.arena.sync_optimizer()         # the re-quantisation reads the fp32 masters
            eng.arena.refresh_fp8()
        eng.bind_inputs(tensors)
        if self._seed_base is None:
            self._seed_base = int(torch.initial_seed())
        eng.prepare_step(self._seed_base + self._step)
        self._step += 1
        eng.run_forward()
        self._last = (eng, tensors)      # keeps the step's input tensors alive until backward
        return eng.losses

    def _run_step(self, node, eager, *args):
        """One step on *args: as the autograd node `node` (an autograd.Function taking model, anchor parameter, *args) when autograd is on
        and a parameter wants a gradient, as `eager(*args)` under no_grad otherwise (always, with node None)."""
        self.materialize()
        anchor = next((p for p in self.parameters() if p.requires_grad), None) if node is not None and torch.is_grad_enabled() else None
        if anchor is not None:
            return node.apply(self, anchor, *args)
        with torch.no_grad():
            return eager(*args)

    def _backward_begin(self, eng, absent=()):
        """Gradient-accumulation bookkeeping shared by the root models.  Parameters of torch-side head modules (`_torch_param_prefixes`) get
        their gradients from autograd (redirected into the arena by a hook).  `absent`: arena names that receive no gradient in this
        backward (a standalone BertModel's pooler whose output got none) -- left as they are, like `unused_params`."""
        arena = eng.arena
        from .optimization import flush_clip
        flush_clip(arena)                   # a clip coefficient no optimizer step has consumed applies to the gradients it was computed for
        if eng.pruned:
            ddp = self._ddp
            if ddp is not None and ddp.reducer.mode == "zero1":
                raise NotImplementedError("DistributedDataParallel(mode='zero1') with frozen parameters: the pruned backward list leaves gradient "
                                          "ranges unwritten, and the sharded step walks every shard; use mode 'allreduce' or 'rs_ag'")
            if arena.grad_plan is None or arena.grad_plan() is not eng:
                # the ranges the pruned list never writes read zero: cleared when this plan takes over (they may hold the gradients of a step
                # before the freeze), not every step -- gradient accumulation adds the whole arena and so keeps them at zero
                for n in eng.pruned:
                    arena.view(n, "grad").zero_()
        arena.grad_plan = weakref.ref(eng)
        skip = self._torch_param_prefixes
        # frozen parameters (requires_grad False: volta/train_utils.py:250-255) get no .grad, as under autograd; the
        # optimizer and clip_grad_norm_ then leave their arena chunks alone
        unused = eng.unused_params          # e.g. the VQA text pooler in pre-training: no launch reads it, .grad stays None
        pairs = [((n, p), g) for (n, p), g in zip(arena.param_list(), arena.grad_views())
                 if p.requires_grad and not (skip and n.startswith(skip)) and n not in unused and n not in absent]
        params, gviews = [x[0] for x in pairs], [x[1] for x in pairs]
        n_have = sum(p.grad is not None for _, p in params)
        accumulate = n_have == len(params)
        if n_have and not accumulate:
            raise RuntimeError("volta_amd: some parameters carry a .grad and some do not; zero_grad() all of them")
        old = None
        if accumulate:
            if not all(p.grad is g or p.grad.data_ptr() == g.data_ptr() for (_, p), g in zip(params, gviews)):
                raise RuntimeError("volta_amd: .grad tensors were replaced by foreign tensors; call zero_grad(set_to_none=True)")
            old = arena.grad.clone()
        return params, gviews, accumulate, old

    def _backward_run(self, eng, state):
        params, gviews, accumulate, old = state
        arena = eng.arena
        skip = self._torch_param_prefixes
        if skip:            # the engine list zero-fills / overwrites only what it owns; torch-side head gradients are already in the arena
            keep = [(g, g.clone()) for (n, _), g in zip(arena.param_list(), arena.grad_views()) if n.startswith(skip)] if accumulate else []
        ddp = self._ddp
        if ddp is not None:
            ddp.run_backward(eng)
        else:
            eng.bwd.run()
        if accumulate:
            from . import _lib as L
            L.check(L.lib.vk_axpy_f32(L.ptr(arena.grad), L.ptr(old), 1.0, arena.total, L.stream_ptr()))
            if skip:
                for g, saved in keep:
                    g.copy_(saved)
        else:
            for (_, p), g in zip(params, gviews):
                p.grad = g

    def _encode_labels(self, B, T, R, dev):
        """Label tensors the plan that encode() runs reads besides the inputs (the pre-training plan: dummies)."""
        return {}

    def encode(self, input_ids, image_feat, image_loc, token_type_ids=None, attention_mask=None, image_attention_mask=None,
               output_all_encoded_layers=False, output_all_attention_masks=False):
        """A nested BertModel's forward, without gradient: (seq_t [B,T,H], seq_v [B,Rv,Hv], pooled_t, pooled_v, attention maps = ([], []));
        with `output_all_encoded_layers` the two sequences are lists with both streams' states after EVERY sub-layer (encoders.py:868-881)."""
        B, T = input_ids.shape
        labels = self._encode_labels(B, T, image_feat.shape[1] - self.add_global_imgfeat, next(self.parameters()).device)
        tensors, B, T, Rv = self._prep_inputs(input_ids, image_feat, image_loc, token_type_ids, attention_mask, image_attention_mask, **labels)
        self._run_step(None, self._engine_forward, tensors, None, output_all_attention_masks and self.config.visualization)
        eng = self._last[0]
        attn_maps = _attention_maps(self.config, eng, output_all_attention_masks)
        H, Hv = self.config.hidden_size, self.config.v_hidden_size
        pt, pv = eng.taps["pooled_t"], eng.taps["pooled_v"]          # None where the fusion method has no such pooler
        if output_all_encoded_layers:
            seq_t = [eng.taps["t%d" % n].view(B, T, H).float() for n in eng.sublayer_ids]
            seq_v = [eng.taps["v%d" % n].view(B, Rv, Hv).float() for n in eng.sublayer_ids]
        else:
            seq_t, seq_v = eng.taps["seq_t"].view(B, T, H).float(), eng.taps["seq_v"].view(B, Rv, Hv).float()
        return seq_t, seq_v, None if pt is None else pt.float(), None if pv is None else pv.float(), attn_maps


class _BackboneStep(torch.autograd.Function):
    """A standalone BertModel's forward as one autograd node.  Outputs (fp32): the final text / vision states, the pooled vectors the fusion
    method has, then with output_all_encoded_layers the states after every sub-layer but the last.  Their gradients re-enter the engine as
    the seeds of its backward list; a gradient autograd does not materialise (None) costs no pass."""

    @staticmethod
    def forward(ctx, model, anchor, tensors, all_layers, maps):
        ctx.set_materialize_grads(False)
        outs = model._backbone_forward(tensors, all_layers, maps)
        ctx.model, ctx.serial, ctx.names = model, model._fwd_serial, [n for n, _ in outs]
        return tuple(t for _, t in outs)

    @staticmethod
    def backward(ctx, *grads):
        ctx.model._backbone_backward(ctx, dict(zip(ctx.names, grads)))
        return None, None, None, None, None


class BertModel(EngineHostModel):
    """Embeddings + gated encoder + poolers (volta/encoders.py:918-1017).

    Inside BertForVLPreTraining / BertForVLTasks it is the parameter container of the root model, and `forward` is the root's `encode()`
    (no gradient).  Constructed on its own it is a root model: it owns its arena and engines, and `forward` runs the engine's forward and,
    under autograd, its backward, seeded by the gradients of whatever torch code consumes the outputs (a custom task head)."""

    _heads_mode = "backbone"
    _arena_prefix = "bert."        # the engine addresses parameters by the names they have inside the root models

    def __init__(self, config):
        super().__init__(config)
        kind = config.image_embeddings
        self.shared_embeddings = kind in M.SHARED
        if config.model != "bert":
            raise NotImplementedError("RoBERTa embeddings are out of scope (SURVEY.md 2.1 #3)")
        if kind in M.DUAL:
            self.embeddings = M.build(M.EMBEDDING_SPECS["text"], config)
            self.v_embeddings = M.build(M.EMBEDDING_SPECS[kind], config)
        elif kind == "vl-bert":
            self.embeddings = M.build_vlbert_embeddings(config)
        elif kind in M.SHARED:
            self.embeddings = M.build(M.EMBEDDING_SPECS[kind], config)
        else:
            raise ValueError("unknown image_embeddings %r" % kind)
        self.encoder = BertEncoder(config)
        self.fusion_method = fm = config.fusion_method
        if fm not in ("sum", "mul", "text", "vl-bert_vqa", "none"):
            raise ValueError("Invalid fusion method: %s" % fm)
        # encoders.py:936-947: "none" has no poolers, "text" / "vl-bert_vqa" (VLBertTextPooler, :610-623) no vision pooler
        if fm != "none":
            self.t_pooler = M.Holder()
            self.t_pooler.add_module("dense", M.LinearParams(config.hidden_size, config.pooler_size))
        if fm in ("sum", "mul"):
            assert config.pooler_size == config.v_pooler_size, "pooler_size != v_pooler_size"
            self.v_pooler = M.Holder()
            self.v_pooler.add_module("dense", M.LinearParams(config.v_hidden_size, config.v_pooler_size))
        M.init_bert_(self, config.initializer_range)
        M.special_init_embeddings_(self.embeddings, kind, config)
        self._init_root_state()          # a root model that builds this BertModel takes its parameters and this state (_adopt)

    def forward(self, input_txt, input_imgs, image_loc, token_type_ids=None, attention_mask=None,
                image_attention_mask=None, output_all_encoded_layers=False, output_all_attention_masks=False):
        """The reference's signature and result (encoders.py:954-1017): (seq_t [B,T,H], seq_v [B,Rv,Hv], pooled_t, pooled_v, attention maps);
        with `output_all_encoded_layers` the two sequences are lists of both streams' states after every sub-layer.  Standalone, the
        outputs are fp32 and differentiable with respect to every parameter; the attention maps are returned DETACHED (no gradient flows
        through them).  Nested in a root model this is the root's `encode()`, without gradient."""
        root = self.__dict__.get("_root")
        if root is not None:
            return root.encode(input_txt, input_imgs, image_loc, token_type_ids, attention_mask, image_attention_mask,
                               output_all_encoded_layers=output_all_encoded_layers, output_all_attention_masks=output_all_attention_masks)
        tensors, B, T, Rv = self._prep_inputs(input_txt, input_imgs, image_loc, token_type_ids, attention_mask, image_attention_mask)
        all_layers = bool(output_all_encoded_layers)
        maps = bool(output_all_attention_masks and self.config.visualization)
        flat = self._run_step(_BackboneStep, lambda *a: [t for _, t in self._backbone_forward(*a)], tensors, all_layers, maps)
        eng = self._last[0]
        out = dict(zip([n for n, _ in self._backbone_outputs(eng, all_layers)], flat))
        attn_maps = _attention_maps(self.config, eng, output_all_attention_masks)
        if all_layers:
            last = eng.sublayer_ids[-1]
            seq_t = [out["t%d" % n] for n in eng.sublayer_ids if n != last] + [out["seq_t"]]
            seq_v = [out["v%d" % n] for n in eng.sublayer_ids if n != last] + [out["seq_v"]]
        else:
            seq_t, seq_v = out["seq_t"], out["seq_v"]
        return seq_t, seq_v, out.get("pooled_t"), out.get("pooled_v"), attn_maps

    # ------------------------------------------------------------------ standalone root model
    def _backbone_outputs(self, eng, all_layers):
        """[(output name, bf16 engine buffer)] in the order of _BackboneStep's outputs."""
        B, T, Rv = eng.B, eng.T, eng.Rv
        H, Hv = self.config.hidden_size, self.config.v_hidden_size
        outs = [("seq_t", eng.taps["seq_t"].view(B, T, H)), ("seq_v", eng.taps["seq_v"].view(B, Rv, Hv))]
        outs += [(n, eng.taps[n]) for n in ("pooled_t", "pooled_v") if eng.taps[n] is not None]
        if all_layers:
            ids = eng.sublayer_ids[:-1]
            outs += [("t%d" % n, eng.taps["t%d" % n].view(B, T, H)) for n in ids] + [("v%d" % n, eng.taps["v%d" % n].view(B, Rv, Hv)) for n in ids]
        return outs

    def _backbone_forward(self, tensors, all_layers, maps):
        from .optimization import flush_clip
        flush_clip(self._arena)      # a pending clip coefficient belongs to the gradients as they are now, before autograd adds to any of them
        self._engine_forward(tensors, attn_maps=maps)
        self._fwd_serial += 1
        return [(n, t.float()) for n, t in self._backbone_outputs(self._last[0], all_layers)]

    def _backbone_backward(self, ctx, grads):
        if getattr(ctx, "done", False):
            raise RuntimeError("volta_amd.BertModel: a second backward through the same forward (its engine state was consumed by the first)")
        if ctx.serial != self._fwd_serial:
            raise RuntimeError("volta_amd.BertModel: this backward belongs to a forward that a later forward of the same model has overtaken; "
                               "its activations are gone (run backward before the next forward)")
        ctx.done = True
        eng, _ = self._last
        # a pooler whose output received no gradient gets none, as under autograd (the engine's pass writes zeros into its arena slots)
        absent = {"bert.%s.dense.%s" % (p, w) for o, p in (("pooled_t", "t_pooler"), ("pooled_v", "v_pooler")) if o in grads and grads[o] is None
                  for w in ("weight", "bias")}
        state = self._backward_begin(eng, absent=absent)
        keep = eng.bind_grads(grads)
        self._backward_run(eng, state)
        del keep


class BertPreTrainingHeads(M.Holder):
    """cls.predictions / cls.bi_seq_relationship / cls.imagePredictions (volta/encoders.py:643-764)."""

    def __init__(self, config, bert_model_embedding_weights):
        super().__init__()
        H, Hv = config.hidden_size, config.v_hidden_size
        pred, tr = M.Holder(), M.Holder()
        tr.add_module("dense", M.LinearParams(H, H))
        tr.add_module("LayerNorm", M.LayerNormParams(H))
        pred.add_module("transform", tr)
        dec = M.Holder()
        dec.weight = bert_model_embedding_weights            # tied (encoders.py:691)
        pred.add_module("decoder", dec)
        pred.bias = nn.Parameter(torch.zeros(bert_model_embedding_weights.size(0)))
        self.add_module("predictions", pred)
        if config.fusion_method not in ("none", "vl-bert_vqa"):            # encoders.py:744-747
            self.add_module("bi_seq_relationship", M.LinearParams(config.pooler_size, 2))
        img, itr = M.Holder(), M.Holder()
        itr.add_module("dense", M.LinearParams(Hv, Hv))
        if config.image_head_ln:
            itr.add_module("LayerNorm", M.LayerNormParams(Hv))
        img.add_module("transform", itr)
        widths = {"0": 1601, "1": 2048, "2": 2048, "3": 1600, "4": 400, "5": 2048, "6": 1601}   # losses.py:129-137
        img.add_module("decoder_dict", nn.ModuleDict({ix: M.LinearParams(Hv, n) for ix, n in widths.items()
                                                       if config.visual_target_weights.get(ix, 0) > 0}))
        self.add_module("imagePredictions", img)
        self.fusion_method = config.fusion_method
        M.init_heads_(self)
        M.init_tied_decoder_(bert_model_embedding_weights)


class _PretrainStep(torch.autograd.Function):
    """One autograd node for the whole model: forward = engine forward list, backward = engine backward list.
    Parameter gradients are written straight into the flat gradient arena and attached as `.grad` views."""

    @staticmethod
    def forward(ctx, model, anchor, tensors):
        ctx.model = model
        return model._losses(tensors)

    @staticmethod
    def backward(ctx, g_lm, g_img, g_nsp):
        ctx.model._engine_backward(g_lm, g_img, g_nsp)
        return None, None, None


class BertForVLPreTraining(EngineHostModel):
    """BERT model with multimodal pre-training heads (volta/encoders.py:1020-1114)."""

    def __init__(self, config):
        super().__init__(config)
        self.bert = BertModel(config)
        self.cls = BertPreTrainingHeads(config, self.bert.embeddings.word_embeddings.weight)
        self.visual_target_weights = config.visual_target_weights
        logger.info("model's visual targets are %s", [ix for ix, w in config.visual_target_weights.items() if w > 0])
        self.tie_weights()
        self._init_root_state()

    def tie_weights(self):
        self._tie_or_clone_weights(self.cls.predictions.decoder, self.bert.embeddings.word_embeddings)

    def _losses(self, tensors):
        losses = self._engine_forward(tensors)
        return losses[0:1].clone(), losses[1:2].clone(), losses[2:3].clone()

    def _engine_backward(self, g_lm, g_img, g_nsp):
        eng, tensors = self._last
        state = self._backward_begin(eng)
        torch.cat([g_lm.reshape(1), g_img.reshape(1), g_nsp.reshape(1)], out=eng.gout)      # one launch, no temporary
        self._backward_run(eng, state)

    # ------------------------------------------------------------------ public API
    def forward(self, input_ids, image_feat, image_loc, token_type_ids=None, attention_mask=None,
                image_attention_mask=None, masked_lm_labels=None, image_label=None, image_cls=None, obj_labels=None,
                obj_confs=None, attr_labels=None, attr_confs=None, image_attrs=None, next_sentence_label=None,
                output_all_attention_masks=False):
        # (with losses the reference returns the three losses only, encoders.py:1111-1112: the attention maps are not part of that result)
        if masked_lm_labels is None and next_sentence_label is None:
            # encoders.py:1113-1114: without text labels and without a masked region every loss is zero and the reference returns the heads' scores
            return self._scores(input_ids, image_feat, image_loc, token_type_ids, attention_mask, image_attention_mask, image_label,
                                output_all_attention_masks)
        if masked_lm_labels is None or image_label is None:
            raise NotImplementedError("the pre-training step needs masked_lm_labels and image_label")
        tensors, B, T, Rv = self._prep_inputs(input_ids, image_feat, image_loc, token_type_ids, attention_mask,
                                              image_attention_mask, masked_lm_labels, image_label, image_cls, next_sentence_label,
                                              obj_labels, obj_confs, attr_labels, attr_confs)
        return self._run_step(_PretrainStep, self._losses, tensors)

    def _scores(self, input_ids, image_feat, image_loc, token_type_ids, attention_mask, image_attention_mask, image_label, output_all_attention_masks=False):
        """The score-returning branch of BertForVLPreTraining.forward (volta/encoders.py:1065-1068,1113-1114): (prediction_scores_t [B,T,V],
        {target: prediction_scores_v [B,Rv,C]}, seq_relationship_score [B,2] or None, attention maps = ([], []), pooled_output or None), the heads
        applied to EVERY position.  Inference only (no gradient, the heads' dropout is the identity); the projections run on the library's GEMM /
        LayerNorm kernels through volta_amd.ops."""
        from . import _lib as L, ops
        if image_label is not None and bool((image_label == 1).any()):
            raise ValueError("masked regions without text labels: the reference returns the losses here, which need masked_lm_labels")
        with torch.no_grad():
            was_training = self.training
            self.eval()
            try:
                seq_t, seq_v, pt, pv, attn_maps = self.encode(input_ids, image_feat, image_loc, token_type_ids, attention_mask, image_attention_mask,
                                                              output_all_attention_masks=output_all_attention_masks)
            finally:
                self.train(was_training)
            eng = self._last[0]
            arena = eng.arena
            W, Pm = (lambda n: arena.view(n, "shadow")), (lambda n: arena.view(n, "master"))
            dev = seq_t.device
            B, T, H = seq_t.shape
            Rv, Hv = seq_v.shape[1], seq_v.shape[2]
            cfg = self.config

            def head(x, rows, K, pre, with_ln, decoders):
                """x bf16 [rows, K] -> transform (dense + GELU (+ LayerNorm)) -> {name: fp32 scores}"""
                h, gp = torch.empty(rows, K, device=dev, dtype=torch.bfloat16), torch.empty(rows, K, device=dev, dtype=torch.bfloat16)
                ops.gemm_grouped(L.NT, L.EPI_GELU, [ops.gemm_problem(x, W(pre + "transform.dense.weight"), h, L.NT, rows, K, K, bias=Pm(pre + "transform.dense.bias"), C2=gp)])
                if with_ln:
                    hn = torch.empty_like(h)
                    mean, rstd = torch.empty(rows, device=dev), torch.empty(rows, device=dev)
                    ops.ln_fwd(h, None, Pm(pre + "transform.LayerNorm.weight"), Pm(pre + "transform.LayerNorm.bias"), hn, None, mean, rstd, rows, K)
                    h = hn
                out = {}
                for name, (wt, bias, C) in decoders.items():
                    Cp = -(-C // 64) * 64
                    sc = torch.empty(rows, Cp, device=dev)
                    ops.gemm_grouped(L.NT, L.EPI_F32, [ops.gemm_problem(h, wt, sc, L.NT, rows, C, K, bias=bias, n_store=Cp)])
                    out[name] = sc[:, :C]
                return out

            xt = eng.taps["seq_t"]
            scores_t = head(xt, B * T, H, "cls.predictions.", True,
                            {"t": (W("bert.embeddings.word_embeddings.weight"), Pm("cls.predictions.bias"), cfg.vocab_size)})["t"].reshape(B, T, -1)
            widths = {"0": 1601, "1": 2048, "2": 2048, "3": 1600, "4": 400, "5": 2048, "6": 1601}
            decs = {ix: (W("cls.imagePredictions.decoder_dict.%s.weight" % ix), Pm("cls.imagePredictions.decoder_dict.%s.bias" % ix), widths[ix])
                    for ix, w in cfg.visual_target_weights.items() if w > 0}
            sv = head(eng.taps["seq_v"], B * Rv, Hv, "cls.imagePredictions.", bool(cfg.image_head_ln), decs)
            scores_v = {ix: t.reshape(B, Rv, -1) for ix, t in sv.items()}
            fm = self.bert.fusion_method
            pooled = None if fm == "none" else (pt * pv if fm == "mul" else pt + pv if fm == "sum" else pt)
            itm = None
            if fm in ("mul", "sum", "text"):
                P = pooled.shape[1]
                pb = pooled.to(torch.bfloat16).contiguous()
                sc = torch.empty(B, 64, device=dev)
                ops.gemm_grouped(L.NT, L.EPI_F32, [ops.gemm_problem(pb, W("cls.bi_seq_relationship.weight"), sc, L.NT, B, 2, P, bias=Pm("cls.bi_seq_relationship.bias"), n_store=64)])
                itm = sc[:, :2]
            return scores_t, scores_v, itm, attn_maps, pooled

    def _encode_labels(self, B, T, R, dev):
        return dict(masked_lm_labels=torch.full((B, T), -1, dtype=torch.int64, device=dev),
                    image_label=torch.full((B, R), -1, dtype=torch.int64, device=dev),
                    image_cls=torch.zeros(B, R, 1601, device=dev), next_sentence_label=torch.zeros(B, dtype=torch.int64, device=dev),
                    obj_labels=torch.zeros(B, R, dtype=torch.int64, device=dev), obj_confs=torch.zeros(B, R, device=dev),
                    attr_labels=torch.zeros(B, R, dtype=torch.int64, device=dev), attr_confs=torch.zeros(B, R, device=dev))


def _attention_maps(config, eng, requested):
    """all_attention_mask of BertEncoder.forward (volta/encoders.py:858-886): empty lists unless requested; one entry per attention
    sub-layer otherwise -- the dictionaries of encoders.py:342-356 under config.visualization, None without it (:357-358)."""
    if not requested:
        return ([], [])
    if config.visualization:
        return eng.attention_maps()
    n = sum(1 for _, typ in M.sublayer_schedule(config) if typ == "attn")
    return ([None] * n, [None] * n)


# ======================================================================================== downstream tasks
class SimpleClassifier(nn.Module):
    """Linear -> GELU -> LayerNorm -> Linear (volta/encoders.py:787-815): the parameter container with the reference's names; the arithmetic
    runs on the HIP engine (engine/heads.py:_heads_tasks), `forward` is kept for reference use on CPU copies only."""

    def __init__(self, in_dim, hid_dim, out_dim, dropout_prob=0.0):
        super().__init__()
        self.logit_fc = nn.Sequential(nn.Linear(in_dim, hid_dim), nn.GELU(), nn.LayerNorm(hid_dim, eps=1e-12), nn.Linear(hid_dim, out_dim))

    def forward(self, hidden_states):
        return self.logit_fc(hidden_states)


class _TaskStep(torch.autograd.Function):
    """Encoder + poolers + the task's classifier as one autograd node: the prediction leaves the engine as fp32 logits, its gradient
    re-enters it as the seed of the backward list."""

    @staticmethod
    def forward(ctx, model, anchor, tensors, task_id, maps):
        ctx.model = model
        return model._predict(tensors, task_id, maps)

    @staticmethod
    def backward(ctx, g_pred):
        model = ctx.model
        eng, _ = model._last
        state = model._backward_begin(eng)
        C = eng.pred_shape[-1]
        eng.d_pred[:, :C].copy_(g_pred.reshape(-1, C))        # the pad columns stay zero
        model._backward_run(eng, state)
        return None, None, None, None, None


_TASK_LOSS_KINDS = {"bce_scaled": 0, "bce_mean": 1, "bce_regions": 2, "ce_options": 3}      # VK_TASK_* of include/volta_hip.h


def _task_loss_args(eng, tensors, target, kind, num_options):
    """vk_task_loss_args over the engine's logits for this step's target; the result buffers live with the engine plan."""
    from . import _lib as L
    code = _TASK_LOSS_KINDS[kind]
    shape, ld = eng.pred_shape, eng.pred.shape[1]
    mask = None
    if kind == "bce_regions":
        if len(shape) != 3:
            raise ValueError("kind 'bce_regions' needs a region-logit task (V-logit); this task predicts %r" % (shape,))
        groups, n = shape[0], shape[1]
        mask = tensors["image_attention_mask"]
    elif len(shape) != 2:
        raise ValueError("kind %r needs a pooled-output task; this task predicts %r" % (kind, shape))
    elif kind == "ce_options":
        if shape[1] != 1 or not num_options or shape[0] % int(num_options):
            raise ValueError("kind 'ce_options' needs a one-score task (VL-logit) and num_options dividing its %d rows" % shape[0])
        groups, n = shape[0] // int(num_options), int(num_options)
    else:
        groups, n = shape
    if kind == "ce_options":
        if target.dtype != torch.int64 or target.numel() != groups:
            raise ValueError("kind 'ce_options' takes an int64 target of %d option indices" % groups)
    elif target.dtype != torch.float32 or target.numel() != groups * n:
        raise ValueError("kind %r takes a float32 target of %d x %d scores, got %s %r" % (kind, groups, n, target.dtype, tuple(target.shape)))
    bufs = eng.task_loss_bufs
    if bufs is None or bufs[2].numel() != groups:
        dev = eng.pred.device
        bufs = eng.task_loss_bufs = (torch.empty(L.lib.vk_task_loss_work_bytes(groups), dtype=torch.uint8, device=dev),
                                     torch.empty(2, dtype=torch.float32, device=dev), torch.empty(groups, dtype=torch.int32, device=dev))
    work, out, amax = bufs
    return L.TaskLossArgs(L.ptr(eng.pred), L.ptr(target), L.ptr(mask), L.ptr(work), L.ptr(out), L.ptr(amax), code, groups, n, ld), out, amax


class _TaskLossStep(torch.autograd.Function):
    """_TaskStep with the task's loss inside the node: the forward list, then vk_task_loss_fwd on the logits where the engine left them;
    backward writes d(loss)/d(logits) x the incoming gradient (read on the device) as bf16 into the engine's seed buffer and runs the
    backward list.  Returns (float[2] = loss, score sum; int32 arg-max per group); only the loss carries a gradient."""

    @staticmethod
    def forward(ctx, model, anchor, tensors, task_id, target, kind, num_options):
        ctx.model, ctx.target = model, target       # the target stays alive until the backward has read it
        ctx.args, res, idx = model._task_loss_forward(tensors, task_id, target, kind, num_options)
        ctx.mark_non_differentiable(idx)
        return res, idx

    @staticmethod
    def backward(ctx, g_res, _g_idx):
        from . import _lib as L
        model = ctx.model
        eng, _ = model._last
        state = model._backward_begin(eng)
        g = g_res.to(torch.float32).contiguous()                    # g[0] = d(objective)/d(loss); the score carries none
        L.check(L.lib.vk_task_loss_bwd(ctx.args, L.ptr(g), L.ptr(eng.d_pred), L.stream_ptr()))
        model._backward_run(eng, state)
        return None, None, None, None, None, None, None


class BertForVLTasks(EngineHostModel):
    """Fine-tuning / evaluation model of the downstream tasks (volta/encoders.py:1117-1206): encoder, poolers, fusion + dropout and the
    task's classifier all run on the HIP engine, forward and backward; `clfs_dict` holds the classifiers' parameters under the reference's
    names and is never called."""

    _heads_mode = "tasks"

    def __init__(self, config, task_cfg, task_ids, dropout_prob=0.1):
        super().__init__(config)
        self.bert = BertModel(config)
        if not 0.0 <= float(dropout_prob) < 1.0:
            raise ValueError("dropout probability has to be between 0 and 1, but got {}".format(dropout_prob))
        self.task_cfg = task_cfg
        task2clf = {}
        for task_id in task_ids:
            task_type = task_cfg[task_id]["type"]
            if task_type in {"VL-classifier", "VL-classifier-GQA"}:
                task2clf[task_id] = SimpleClassifier(config.pooler_size, config.clf_hidden_size, task_cfg[task_id]["num_labels"])
            elif task_type == "VL-binary-classifier":
                task2clf[task_id] = SimpleClassifier(config.pooler_size * 2, config.clf_hidden_size, 2)
            elif task_type == "VL-tri-classifier":
                task2clf[task_id] = nn.Linear(config.pooler_size, 3)
            elif task_type == "VL-logit":
                task2clf[task_id] = nn.Linear(config.pooler_size, 1)
            elif task_type.startswith("V-logit"):
                if task_cfg[task_id].get("num_clf_layers", 1) == 2:
                    task2clf[task_id] = nn.Sequential(nn.Linear(config.v_hidden_size, config.v_hidden_size), nn.GELU(),
                                                      nn.Dropout(config.v_attention_probs_dropout_prob, inplace=False),
                                                      nn.Linear(config.v_hidden_size, 1))
                else:
                    task2clf[task_id] = nn.Linear(config.v_hidden_size, 1)
            else:
                raise ValueError("Undefined task type: %s" % task_type)
        self.clfs_dict = nn.ModuleDict(task2clf)
        self.fusion_method = config.fusion_method
        for mod in self.clfs_dict.modules():                     # the outer apply(init_weights) of the reference (utils.py:377-389)
            if isinstance(mod, nn.Linear):
                mod.weight.data.normal_(mean=0.0, std=config.initializer_range)
                if mod.bias is not None:
                    mod.bias.data.zero_()
            elif isinstance(mod, nn.LayerNorm):
                mod.bias.data.zero_()
                mod.weight.data.fill_(1.0)
        self._init_root_state(task_dropout=dropout_prob)      # nn.Dropout(dropout_prob) of the reference (encoders.py:1122): an engine op here

    def task_loss(self, input_txt, input_imgs, image_loc, task_id, token_type_ids=None, attention_mask=None, image_attention_mask=None,
                  target=None, *, kind, num_options=None):
        """The model and the task's loss in one step (what ForwardModelsTrain / ForwardModelsVal compute behind `forward`,
        volta/task_utils.py:140-281): returns (loss, score_sum, row_argmax) -- 0-dim fp32 device tensors and an int32 vector with the
        arg-max of every group.  The logits never leave the engine; `loss` is differentiable with respect to every trainable parameter.
        kind: "bce_scaled" (BCE-with-logits mean x C: VL-classifier, VL-classifier-GQA), "bce_mean" (plain mean: VL-binary-classifier,
        VL-tri-classifier), "bce_regions" (V-logit: BCE over the masked region scores x regions) or "ce_options" (VL-logit: cross-entropy
        over `num_options` consecutive samples, int64 target)."""
        res, idx = self._task_loss(input_txt, input_imgs, image_loc, task_id, token_type_ids, attention_mask, image_attention_mask, target, kind, num_options)
        return res[0], res[1].detach(), idx

    def _task_loss(self, input_txt, input_imgs, image_loc, task_id, token_type_ids, attention_mask, image_attention_mask, target, kind, num_options):
        """task_loss with loss and score still in one float[2] tensor (ForwardModelsVal reads both with one transfer)"""
        if task_id not in self.task_cfg or task_id not in self.clfs_dict:
            raise KeyError("unknown task id %r" % (task_id,))
        if kind not in _TASK_LOSS_KINDS:
            raise ValueError("kind %r (%s)" % (kind, " | ".join(_TASK_LOSS_KINDS)))
        if target is None:
            raise ValueError("task_loss needs the target")
        tensors, B, T, Rv = self._prep_inputs(input_txt, input_imgs, image_loc, token_type_ids, attention_mask, image_attention_mask)
        dev = tensors["input_ids"].device
        target = target.to(device=dev).contiguous()
        return self._run_step(_TaskLossStep, lambda *a: self._task_loss_forward(*a)[1:], tensors, task_id, target, kind, num_options)

    def _task_loss_forward(self, tensors, task_id, target, kind, num_options):
        """The forward list of `task_id`'s plan, then vk_task_loss_fwd on its logits: (the launch's arguments, float[2], int32 arg-max)."""
        from . import _lib as L
        self._engine_forward(tensors, task_id)
        args, out, amax = _task_loss_args(self._last[0], tensors, target, kind, num_options)
        L.check(L.lib.vk_task_loss_fwd(args, L.stream_ptr()))
        return args, out.clone(), amax.clone()

    def _predict(self, tensors, task_id, maps):
        """The forward list of `task_id`'s plan (the plan whose head is this task's classifier): its logits in fp32."""
        self._engine_forward(tensors, task_id, maps)
        eng = self._last[0]
        C = eng.pred_shape[-1]
        return eng.pred[:, :C].reshape(eng.pred_shape).clone()

    def forward(self, input_txt, input_imgs, image_loc, task_id, token_type_ids=None, attention_mask=None,
                image_attention_mask=None, output_all_encoded_layers=False, output_all_attention_masks=False):
        if task_id not in self.task_cfg or task_id not in self.clfs_dict:
            raise KeyError("unknown task id %r" % (task_id,))
        tensors, B, T, Rv = self._prep_inputs(input_txt, input_imgs, image_loc, token_type_ids, attention_mask, image_attention_mask)
        maps = bool(output_all_attention_masks and self.config.visualization)
        vil_prediction = self._run_step(_TaskStep, self._predict, tensors, task_id, maps)
        attn_maps = _attention_maps(self.config, self._last[0], output_all_attention_masks)
        if self.task_cfg[task_id]["type"].startswith("V-logit"):   # padded regions are masked out of the region scores (encoders.py:1198-1199)
            mask = tensors["image_attention_mask"].to(vil_prediction.dtype)
            vil_prediction = vil_prediction + ((1.0 - mask) * -10000.0).unsqueeze(2)
        return vil_prediction, None, None, attn_maps
