"""Position-independent text signatures of the step engine's plans, built on the CPU (no GPU needed: the plan builder only takes
addresses and calls host helpers of the library).

  python tools/plan_signature.py                 write tests/golden/plan_signatures.json ({plan id: sha256 of its text})
  python tools/plan_signature.py --check         compare with that file; on a mismatch print a unified diff around the first differing ops
                                                 (the expected text is rendered from the tree at --base, default .base)
  python tools/plan_signature.py --dump DIR      also write the full texts, one file per plan
  python tools/plan_signature.py --tree PATH     import volta_amd from another checkout (the `.base` worktree of tools/ab_bench.sh)
  python tools/plan_signature.py --only REGEX    restrict the matrix (not with a golden write)

One text holds the buffer table, every op of the forward and backward lists with the structures behind it (walked over the ctypes
`_fields_`; every device address printed as `label+byte offset`) and the plan's host-side surface (patched input sites, seeds, taps,
stage marks, dropout sites).  tests/test_plan_signature_cpu.py runs the same matrix against the committed hashes."""
import argparse
import bisect
import ctypes as C
import difflib
import hashlib
import importlib.util
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_signatures.json")
B, T, RV = 2, 20, 37                    # the tiny plans' shape
FAMILIES = ("vilbert", "lxmert", "uniter", "visualbert", "vlbert")
UNRESOLVED = "UNRESOLVED"


def _test_module(name):
    spec = importlib.util.spec_from_file_location("_plan_sig_" + name, os.path.join(ROOT, "tests", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ======================================================================================== rendering
class Renderer:
    """Renders one built StepEngine.  `unresolved` counts the addresses no interval of the table covers."""

    def __init__(self, eng):
        import torch
        from volta_amd import _lib as L
        self.eng, self.L, self.torch = eng, L, torch
        self.unresolved = 0
        arena = eng.arena
        spans = [("buf:" + name, t) for name, t in eng.bufs.items()] + [("seed", eng.seed)]
        spans += [(which, getattr(arena, which)) for which in ("master", "shadow", "grad")]
        for w, q, sc in arena.fp8_sites.values():
            off = (w.data_ptr() - arena.master.data_ptr()) // 4
            spans += [("fp8q:%d" % off, q), ("fp8s:%d" % off, sc)]
        table = sorted((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size(), label) for label, t in spans if t.numel())
        self.starts = [s for s, _, _ in table]
        self.table = table
        self.kept = {}
        for plan_keep in (eng.keep, eng.fwd.keep, eng.bwd.keep):
            for obj in plan_keep:
                if isinstance(obj, (C.Structure, C.Array)):
                    self.kept[C.addressof(obj)] = obj
        self.where = {}              # address of a rendered structure -> ["fwd[3].a", ...]
        self.path = None

    def addr(self, v):
        if not v:
            return "null"
        i = bisect.bisect_right(self.starts, v) - 1
        if i >= 0 and v < self.table[i][1]:
            return "%s+%d" % (self.table[i][2], v - self.table[i][0])
        self.unresolved += 1
        return "%s:%#x" % (UNRESOLVED, v)

    def pointer(self, v, depth):
        if v and v in self.kept:
            return "&" + self.value(self.kept[v], depth + 1)
        return self.addr(v)

    def value(self, o, depth=0):
        if o is None:
            return "null"
        if isinstance(o, self.torch.Tensor):
            return self.addr(o.data_ptr())
        if isinstance(o, bool):
            return str(int(o))
        if isinstance(o, int):
            return self.addr(o)
        if isinstance(o, C.Structure):
            if self.path is not None:
                self.where.setdefault(C.addressof(o), []).append(self.path)
            parts = []
            for fname, ftype in o._fields_:
                parts.append("%s=%s" % (fname, self.field(getattr(o, fname), ftype, depth)))
            return "%s{%s}" % (type(o).__name__, ", ".join(parts))
        if isinstance(o, C.Array):
            return "[%s]" % ", ".join(self.field(o[i], o._type_, depth) for i in range(len(o)))
        raise TypeError("plan signature: cannot render %r" % (o,))

    def field(self, v, ftype, depth):
        if ftype is self.L.c_p:
            return self.pointer(v, depth)
        if isinstance(v, (C.Structure, C.Array)):
            return self.value(v, depth)
        if isinstance(v, float):
            return repr(v)
        if isinstance(v, bytes):
            return repr(v)
        return str(int(v))

    def ops(self, tag, plan):
        out = []
        for i, (kind, i0, i1, i2, a, b, c) in enumerate(plan.ops):
            out.append("%s[%d] kind=%d i0=%d i1=%d i2=%d" % (tag, i, kind, i0, i1, i2))
            for slot, o in (("a", a), ("b", b), ("c", c)):
                if o is not None:
                    self.path = "%s[%d].%s" % (tag, i, slot)
                    out.append("  %s: %s" % (slot, self.value(o)))
                    self.path = None
        return out

    def label(self, t):
        return "null" if t is None else self.addr(t.data_ptr())

    def text(self):
        eng = self.eng
        out = ["# buffers"]
        for name in sorted(eng.bufs):
            t = eng.bufs[name]
            out.append("%s %s %s" % (name, tuple(t.shape), str(t.dtype).replace("torch.", "")))
        out.append("# forward")
        out += self.ops("fwd", eng.fwd)
        out.append("# backward")
        out += self.ops("bwd", eng.bwd)
        out.append("# inputs")
        for name in sorted(eng.inputs):
            for struct, fname, index in eng.inputs[name]:
                where = self.where.get(C.addressof(struct))
                if not where:                              # a structure no op reaches would be patched for nothing
                    self.unresolved += 1
                    where = [UNRESOLVED + ":" + type(struct).__name__]
                out.append("%s -> %s %s%s" % (name, " ".join(where), fname, "" if index is None else "[%d]" % index))
        out.append("# grad_seeds")
        for name in sorted(eng.grad_seeds):
            out.append("%s -> %s" % (name, self.addr(eng.grad_seeds[name].dst)))
        out.append("# taps")
        for name in sorted(eng.taps):
            out.append("%s -> %s" % (name, self.label(eng.taps[name])))
        out.append("# surface")
        for attr in ("bwd_marks", "fwd_sub_start", "fwd_heads_start", "site", "nce_site", "score_classes", "pred_shape"):
            if hasattr(eng, attr):
                out.append("%s = %r" % (attr, getattr(eng, attr)))
        if hasattr(eng, "param_ready_stage"):
            out.append("param_ready_stage = %s" % json.dumps(eng.param_ready_stage, sort_keys=True))
        out.append("unused_params = %r" % (sorted(eng.unused_params),))
        for attr in ("score_out", "pred", "d_pred"):
            if hasattr(eng, attr):
                out.append("%s = %s" % (attr, self.label(getattr(eng, attr))))
        if hasattr(eng, "score_x8"):
            x8 = eng.score_x8
            out.append("score_x8 = %s" % ("null" if x8 is None else "(%s, %s)" % (self.label(x8[0]), self.label(x8[1]))))
        for name, t, side in getattr(eng, "pair_inputs", ()):
            out.append("pair_input %s -> %s side %d" % (name, self.label(t), side))
        for info in eng.attn_map_info:
            out.append("attn_map n=%d nh=%d dh=%d Ha=%s qkv=%s probs=%s" % (
                info["n"], info["nh"], info["dh"], sorted(info["Ha"].items()),
                [(m, self.label(t)) for m, t in sorted(info["qkv"].items())], [(ij, self.label(t)) for ij, t in sorted(info["probs"].items())]))
        return "\n".join(out) + "\n"


def render(eng):
    """(text, number of unresolved addresses) of one built engine."""
    r = Renderer(eng)
    return r.text(), r.unresolved


# ======================================================================================== the matrix
class Matrix:
    """The fixed list of plans.  `entries` = [(plan id, model key, StepEngine keyword arguments)]; models and their arenas are built on
    first use and shared by the plans of one model."""

    def __init__(self):
        eng_t, var_t, task_t = _test_module("test_engine_gpu"), _test_module("test_variants_gpu"), _test_module("test_tasks_gpu")
        self.configs, self.variants, self.task_cfg = eng_t.CONFIGS, var_t.VARIANTS, task_t.TASK_CFG
        self.models = {}
        e = self.entries = []
        shape = dict(B=B, T=T, Rv=RV)
        for name in self.configs:
            for mode, kw in (("train-bf16", dict(train=True)), ("train-fp8", dict(train=True, fp8=True)), ("eval-bf16", dict(train=False))):
                e.append(("pretrain/%s/%s" % (name, mode), ("pretrain", name), dict(shape, **kw)))
        for name in self.variants:
            e.append(("variant/%s/train-bf16" % name, ("pretrain", name), dict(shape, train=True)))
        e.append(("variant/wide_vilbert/train-fp8", ("pretrain", "wide_vilbert"), dict(shape, train=True, fp8=True)))       # refused
        for name in ("vilbert", "wide_vilbert"):
            e.append(("maps/%s/eval" % name, ("pretrain", name), dict(shape, train=False, attn_maps=True)))
        for name in FAMILIES:
            for task in list(self.task_cfg) + [None]:
                for train in (True, False):
                    kw = dict(shape, train=train, heads="tasks", task=(task, self.task_cfg[task]) if task else None)
                    e.append(("tasks/%s/%s/%s" % (name, task or "none", "train" if train else "eval"), ("tasks", name), kw))
        for name in FAMILIES:
            e.append(("backbone/%s/train" % name, ("backbone", name), dict(shape, train=True, heads="backbone")))
        for name in FAMILIES:
            for head in ("TASK8", None):
                for part in ("text", "image", "pair"):          # a part split_plan does not allow is refused: recorded as that
                    for dtype in ("bf16", "fp8"):
                        kw = dict(shape, train=False, heads="score", part=part, projection_dtype=dtype, split="split",
                                  task=("TASK8", self.task_cfg["TASK8"]) if head and part == "pair" else None)
                        e.append(("score/%s/%s/%s/%s" % (name, head or "itm", part, dtype), ("tasks" if head else "pretrain", name), kw))
        e.append(("full/ctrl_vilbert_base/train-bf16", ("pretrain", "ctrl_vilbert_base.json"), dict(B=256, T=20, Rv=37, train=True)))
        e.append(("full/ctrl_vl-bert_base/train-fp8", ("pretrain", "ctrl_vl-bert_base.json"), dict(B=256, T=20, Rv=101, train=True, fp8=True)))
        assert len({pid for pid, _, _ in e}) == len(e)

    def ids(self):
        return [pid for pid, _, _ in self.entries]

    def model(self, key):
        """(config, arena) of one model, on the CPU."""
        if key not in self.models:
            import torch
            from volta_amd.config import BertConfig
            from volta_amd.engine import ParamArena
            from volta_amd import modeling
            kind, name = key
            if name.endswith(".json"):
                cfg = BertConfig.from_json_file(os.path.join(ROOT, "config", name))
            else:
                cd = self.configs[name] if name in self.configs else self.variants[name]
                cfg = BertConfig.from_dict(dict(cd, clf_hidden_size=1536))
            if kind == "tasks":
                model = modeling.BertForVLTasks(cfg, self.task_cfg, list(self.task_cfg))
            else:
                model = (modeling.BertModel if kind == "backbone" else modeling.BertForVLPreTraining)(cfg)
            self.models[key] = (cfg, ParamArena(model, torch.device("cpu"), prefix=model._arena_prefix))
        return self.models[key]

    def build(self, pid):
        """The built engine of one entry, or the exception its constructor raised."""
        from volta_amd.engine import StepEngine
        from volta_amd.retrieval import split_plan
        _, key, kw = next(x for x in self.entries if x[0] == pid)
        cfg, arena = self.model(key)
        kw = dict(kw)
        if kw.get("split") == "split":
            kw["split"] = split_plan(cfg)
        try:
            return StepEngine(cfg, arena, kw.pop("B"), kw.pop("T"), kw.pop("Rv"), kw.pop("train"), **kw)
        except (ValueError, NotImplementedError) as exc:
            return exc

    def text(self, pid):
        """(text, unresolved count): the plan's rendering, or the refusal's type and message."""
        eng = self.build(pid)
        key = next(k for p, k, _ in self.entries if p == pid)
        if key[1].endswith(".json"):          # a full-size model serves one plan: its arenas (about 1 GB each) are not kept
            del self.models[key]
        if isinstance(eng, Exception):
            return "refused: %s: %s\n" % (type(eng).__name__, eng), 0
        return render(eng)


def sha(text):
    return hashlib.sha256(text.encode()).hexdigest()


def first_difference(want, got, context=3):
    """Unified diff of two texts around their first differing lines."""
    a, b = want.splitlines(), got.splitlines()
    i = next((k for k, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    lo = max(0, i - context)
    return "\n".join(difflib.unified_diff(a[lo:i + 40], b[lo:i + 40], "base tree (from line %d)" % (lo + 1), "this tree", lineterm="", n=context))


def diff_against(base, pid, text):
    """The golden holds hashes only: the text to diff a mismatch against is rendered from the `base` tree, in a process of its own."""
    if not os.path.isdir(os.path.join(base, "volta_amd")):
        return "(no tree at %s to render the expected text from: see --base)" % base
    with tempfile.TemporaryDirectory() as d:
        subprocess.run([sys.executable, os.path.abspath(__file__), "--tree", base, "--dump", d, "--only", "^%s$" % re.escape(pid)],
                       stdout=subprocess.DEVNULL, check=False)
        ref = os.path.join(d, pid.replace("/", "__") + ".txt")
        return first_difference(open(ref).read(), text) if os.path.exists(ref) else "(the base tree did not render this plan)"


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--dump", metavar="DIR")
    ap.add_argument("--tree", metavar="PATH")
    ap.add_argument("--only", metavar="REGEX")
    ap.add_argument("--base", metavar="PATH", default=os.path.join(ROOT, ".base"), help="--check: the tree whose texts a mismatch is diffed against")
    args = ap.parse_args(argv)
    sys.path.insert(0, os.path.abspath(args.tree) if args.tree else ROOT)
    if args.tree:
        sys.path.append(ROOT)
    matrix = Matrix()
    ids = [pid for pid in matrix.ids() if not args.only or re.search(args.only, pid)]
    golden = json.load(open(GOLDEN)) if args.check else {}
    if args.dump:
        os.makedirs(args.dump, exist_ok=True)
    hashes, bad = {}, 0
    for pid in ids:
        text, unresolved = matrix.text(pid)
        hashes[pid] = sha(text)
        if args.dump:
            open(os.path.join(args.dump, pid.replace("/", "__") + ".txt"), "w").write(text)
        if unresolved:
            bad += 1
            print("%s: %d unresolved addresses" % (pid, unresolved))
        if args.check and golden.get(pid) != hashes[pid]:
            bad += 1
            print("%s: signature differs from the golden" % pid)
            print(diff_against(args.base, pid, text))
    if args.check:
        missing = [] if args.only else sorted(set(golden) - set(hashes))
        for pid in missing:
            print("%s: in the golden, not in the matrix" % pid)
        bad += len(missing)
        print("%d plans checked, %d problems" % (len(ids), bad))
    elif not bad and not args.only:
        with open(GOLDEN, "w") as fh:
            json.dump(hashes, fh, indent=0, sort_keys=True)
            fh.write("\n")
        print("wrote %d hashes to %s" % (len(hashes), os.path.relpath(GOLDEN, ROOT)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
