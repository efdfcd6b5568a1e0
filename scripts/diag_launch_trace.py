"""Record every C-ABI call of the U-Net engine, per configuration, as one JSON line each — to compare two trees of the
host code (a refactor against its parent) launch for launch.

The loaded library handle (``deadtrees_amd._lib._lib``) is replaced by a recording proxy BEFORE a model is built, so the
script needs nothing from the tree under test but its public surface.  A line holds: the entry point; scalars by value;
``ConvDesc`` / ``LossCfg`` by field; ``BnBwdFuse`` as its null pattern; every pointer argument (known from
``_lib.SIGNATURES``) as null, as buffer name + byte offset when it lies inside ``flat_params``, the gradient buffer or
``bn_state``, else as "device"; the stream as main or side; the return value.  Per configuration it also prints a SHA-256
of logits (class map for inference), gradient buffer, ``bn_state`` and parameters.  The last line of a configuration is its
extra output: the ``profile`` list (name, FLOPs, bytes) of a profiled one, (key, shape, dtype, SHA-256) of every tensor of
``engine.trace`` in insertion order of a traced one, the error of one the tree refuses (``{"refused": ...}``), the
``recal_launches`` of a recalibration, hashes of what an inference call returns.

Usage (GPU box, a few seconds per configuration at B = 2 / 64 x 64):
    python scripts/diag_launch_trace.py OUTDIR [configuration ...]      -> OUTDIR/<configuration>.jsonl, OUTDIR/hashes.json
    python scripts/diag_launch_trace.py --compare DIR_A DIR_B [--trace-only CONFIG ...]
Point the tree under test at another tree's library with DT_HIP_LIB; run the script that lies in (or is copied next to) the
tree it should import.  Configurations whose hashes differ between two runs of the SAME tree (bit-reproducibility is
tested at the bench sizes, not at 64 x 64) are compared by trace only: name them after --trace-only."""
import ctypes as C
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, S = 2, 64
KINDS = ("unet", "resunet", "unetplusplus")


class Recorder:
    """stands in for the ctypes library handle: every entry point of SIGNATURES is recorded, then called"""

    def __init__(self, lib, signatures, main_stream: int = 0):
        self._lib, self._sigs, self._main = lib, signatures, main_stream
        self.lines, self.buffers = [], {}          # buffers: {name: (address, bytes)}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        sig = self._sigs.get(name)
        if sig is None:
            return fn

        def call(*args):
            line = {"fn": name, "args": [self._describe(t, a, i == len(args) - 1) for i, (t, a) in enumerate(zip(sig[1], args))]}
            ret = fn(*args)
            line["ret"] = ret.decode() if isinstance(ret, bytes) else ret
            self.lines.append(json.dumps(line))
            return ret

        self.__dict__[name] = call
        return call

    def _describe(self, typ, a, last: bool):
        if typ is C.c_void_p:
            v = a.value if isinstance(a, C.c_void_p) else a
            if last:
                return "main" if (v or 0) == self._main else "side"
            if not v:
                return "null"
            for name, (lo, n) in self.buffers.items():
                if lo <= v < lo + n:
                    return [name, v - lo]
            return "device"
        obj = getattr(a, "_obj", a)                 # byref(x) -> x
        if isinstance(obj, C.Structure):
            vals = {f: getattr(obj, f) for f, _ in obj._fields_}
            if type(obj).__name__ == "BnBwdFuse":
                return "".join("1" if vals[f] else "0" for f, _ in obj._fields_)
            return vals
        if hasattr(typ, "contents") or isinstance(obj, C._SimpleCData):   # POINTER(c_int) results, host float arrays
            return "host"
        return a.decode() if isinstance(a, bytes) else a


def sha(t):
    import torch
    if t is None:
        return None
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def build(kind, rec):
    import torch
    from deadtrees_amd.network.unet import UNetHIP
    m = UNetHIP(decoder=kind)
    m.reset_parameters(seed=0)
    m = m.to("cuda")
    eng, kept = m.engine, {}
    for name in ("forward", "forward_bf16_train", "forward_bf16_eval"):     # keep the logits of the last forward alive

        def tapped(*a, _fn=getattr(eng, name), **k):
            out = _fn(*a, **k)
            kept["logits"] = out[0] if isinstance(out, tuple) else out
            return out
        setattr(eng, name, tapped)
    g = m._grad_buffer()
    rec.buffers = {n: (t.data_ptr(), t.numel() * t.element_size())
                   for n, t in (("flat_params", m.flat_params.data), ("grads", g), ("bn_state", m.bn_state))}
    return m, kept


def configurations():
    """{name: (decoder kind, environment for the engine's construction, action(model, img, mask) -> extra output)}"""
    import torch
    from deadtrees_amd.trainer import HipTrainer

    def step(precision, prepare=None, profile=False, trace=False):
        def run(m, img, mask):
            if profile:
                m.engine.profile = []
            if trace:
                m.engine.trace = {}
            try:
                if prepare:
                    prepare(m)
                HipTrainer(m, precision=precision).step(img, mask)
            except (NotImplementedError, RuntimeError) as e:      # a configuration the tree refuses: refused alike
                return {"refused": f"{type(e).__name__}: {e}"}
            finally:
                prof, m.engine.profile = m.engine.profile, None
                traced, m.engine.trace = m.engine.trace, None
            if trace:       # every traced tensor in insertion order
                return [[k, list(t.shape), str(t.dtype), sha(t)] for k, t in traced.items()]
            return None if prof is None else [[p[0], p[1], p[4]] for p in prof]
        return run

    def predict(precision, profile=False):
        def run(m, img, mask):
            if profile:
                m.engine.profile = []
            cls = m.predict_classes(img, dtype="uint8", precision=precision)
            prof, m.engine.profile = m.engine.profile, None
            return {"classes": sha(cls), "profile": None if prof is None else [[p[0], p[1], p[4]] for p in prof]}
        return run

    def recal(precision):
        def run(m, img, mask):
            m.recalibrate_batch(img, precision)
            m.recalibrate_batch(img, precision)
            return [list(x) for x in m.engine.recal_launches]
        return run

    def frozen_eval(m):
        m.encoder.requires_grad_(False)
        m.encoder.eval()

    def predict_nhwc(precision):
        return lambda m, img, mask: {"classes": sha(m.predict_classes(img.permute(0, 2, 3, 1).contiguous(), dtype="uint8",
                                                                      precision=precision, nhwc=True))}

    def predict_twice(m, img, mask):       # the second call of a precision skips the eval-affine launches
        return [sha(m.predict_logits(img, precision=p)) for p in ("fp32", "fp32", "bf16", "bf16")]

    def eval_head(precision):
        def run(m, img, mask):
            head = m.engine.forward_bf16_eval_head if precision == "bf16" else m.engine.forward_eval_head
            acc, counts, am, err = head(img, m.flat_params.detach(), m.bn_state, mask, want_argmax=True)
            return [sha(acc), sha(counts), sha(am), int(err)]
        return run

    def nograd_forward(train):
        def run(m, img, mask):
            m.train(train)
            with torch.no_grad():
                return {"logits": sha(m(img))}
        return run

    def corner(action):                    # 32 x 32: the stem output is 16 wide -> the fp32 stem kernel with bf16 output
        return lambda m, img, mask: action(m, img[:, :, :32, :32].contiguous(), mask[:, :32, :32].contiguous())

    cfg = {}
    for kind in KINDS:
        cfg[f"{kind}.step_fp32"] = (kind, {}, step("fp32"))
        cfg[f"{kind}.step_bf16"] = (kind, {}, step("bf16"))
        cfg[f"{kind}.predict_fp32"] = (kind, {}, predict("fp32"))
        cfg[f"{kind}.predict_bf16"] = (kind, {}, predict("bf16"))
        cfg[f"{kind}.traced_step_fp32"] = (kind, {}, step("fp32", trace=True))
        cfg[f"{kind}.traced_step_bf16"] = (kind, {}, step("bf16", trace=True))
        if kind != "unet":
            cfg[f"{kind}.frozen_eval_encoder_step_fp32"] = (kind, {}, step("fp32", frozen_eval))
            cfg[f"{kind}.frozen_eval_encoder_step_bf16"] = (kind, {}, step("bf16", frozen_eval))
    cfg["unet.direct_step_fp32"] = ("unet", {}, step("fp32", lambda m: setattr(m.engine, "winograd", False)))
    cfg["unet.frozen_eval_encoder_step_fp32"] = ("unet", {}, step("fp32", frozen_eval))
    cfg["unet.frozen_eval_encoder_step_bf16"] = ("unet", {}, step("bf16", frozen_eval))
    cfg["unet.eval_encoder_step_fp32"] = ("unet", {}, step("fp32", lambda m: m.encoder.eval()))
    cfg["unet.recalibrate_fp32"] = ("unet", {}, recal("fp32"))
    cfg["unet.recalibrate_bf16"] = ("unet", {}, recal("bf16"))
    cfg["unet.virtual_activations_step_fp32"] = ("unet", {"DT_MATERIALIZE_Z1": "0", "DT_MATERIALIZE_Z2": "0"}, step("fp32"))
    cfg["unet.no_bn_fuse_step_fp32"] = ("unet", {"DT_NO_BN_FUSE": "1"}, step("fp32"))
    cfg["unet.no_join_fuse_step_fp32"] = ("unet", {"DT_FUSE_JOIN_FP32": "0"}, step("fp32"))
    cfg["unet.no_pool_bn_step_fp32"] = ("unet", {"DT_FUSE_POOL_BN": "0"}, step("fp32"))
    cfg["unet.no_pool_bn_step_bf16"] = ("unet", {"DT_FUSE_POOL_BN": "0"}, step("bf16"))
    cfg["unet.no_overlap_step_fp32"] = ("unet", {"DT_OVERLAP_WGRAD": "0"}, step("fp32"))
    cfg["unet.overlap_step_bf16"] = ("unet", {"DT_OVERLAP_WGRAD_BF16": "1"}, step("bf16"))
    cfg["unet.profiled_step_fp32"] = ("unet", {}, step("fp32", profile=True))
    cfg["unet.profiled_step_bf16"] = ("unet", {}, step("bf16", profile=True))
    cfg["unet.profiled_predict_fp32"] = ("unet", {}, predict("fp32", profile=True))
    cfg["unet.profiled_predict_bf16"] = ("unet", {}, predict("bf16", profile=True))
    # what the forward schedule has beyond a step and a prediction
    for kind in KINDS:
        cfg[f"{kind}.predict_twice"] = (kind, {}, predict_twice)
        cfg[f"{kind}.eval_head_fp32"] = (kind, {}, eval_head("fp32"))
        cfg[f"{kind}.eval_head_bf16"] = (kind, {}, eval_head("bf16"))
        if kind != "unet":
            cfg[f"{kind}.recalibrate_fp32"] = (kind, {}, recal("fp32"))
            cfg[f"{kind}.recalibrate_bf16"] = (kind, {}, recal("bf16"))
    cfg["efficientunetplusplus.predict_fp32"] = ("efficientunetplusplus", {}, predict("fp32"))
    cfg["efficientunetplusplus.eval_head_fp32"] = ("efficientunetplusplus", {}, eval_head("fp32"))
    cfg["unet.predict_nhwc_fp32"] = ("unet", {}, predict_nhwc("fp32"))
    cfg["unet.predict_nhwc_bf16"] = ("unet", {}, predict_nhwc("bf16"))
    cfg["unet.no_fuse_eval_predict_fp32"] = ("unet", {"DT_FUSE_EVAL": "0"}, predict("fp32"))
    cfg["unet.direct_predict_fp32"] = ("unet", {"DT_FP32_WINOGRAD": "0"}, predict("fp32"))
    cfg["unet.nograd_train_forward_fp32"] = ("unet", {}, nograd_forward(True))
    cfg["unet.nograd_eval_forward_fp32"] = ("unet", {}, nograd_forward(False))
    cfg["unet.no_mat_z1_step_bf16"] = ("unet", {"DT_BF16_MAT_Z1": "0"}, step("bf16"))
    cfg["unet.no_mat_dec_step_bf16"] = ("unet", {"DT_BF16_MAT_DEC": "0"}, step("bf16"))
    cfg["unet.images_unfused_step_bf16"] = ("unet", {"DT_BF16_IMAGES_FUSED": "0"}, step("bf16"))
    cfg["unet.corner32_step_bf16"] = ("unet", {}, corner(step("bf16")))
    cfg["unet.corner32_predict_bf16"] = ("unet", {}, corner(predict("bf16")))
    cfg["unet.eval_encoder_step_bf16"] = ("unet", {}, step("bf16", lambda m: m.encoder.eval()))     # refused
    return cfg


def record(outdir, names):
    import torch
    from deadtrees_amd import _lib
    from deadtrees_amd.data.synthetic import synth_batch
    rec = Recorder(_lib.load(), _lib.SIGNATURES, torch.cuda.default_stream().cuda_stream)
    _lib._lib = rec
    cfg = configurations()
    os.makedirs(outdir, exist_ok=True)
    img, mask = synth_batch(B, S, S, 3, 2, seed=4321)
    img, mask = img.cuda(), mask.cuda()
    hashes = {}
    for name in names or list(cfg):
        kind, env, action = cfg[name]
        os.environ.update(env)
        try:
            m, kept = build(kind, rec)
        finally:
            for k in env:
                del os.environ[k]
        rec.lines = []
        extra = action(m, img, mask)
        torch.cuda.synchronize()
        hashes[name] = {"logits": sha(kept.get("logits")), "grads": sha(m._grad_buffer()), "bn_state": sha(m.bn_state),
                        "params": sha(m.flat_params)}
        with open(os.path.join(outdir, name + ".jsonl"), "w") as f:
            f.write("\n".join(rec.lines) + "\n")
            f.write(json.dumps({"extra": extra}) + "\n")
        print(name, len(rec.lines), "calls", json.dumps(hashes[name]), flush=True)
        del m, kept
    with open(os.path.join(outdir, "hashes.json"), "w") as f:
        json.dump(hashes, f, indent=1)


def compare(dir_a, dir_b, trace_only):
    ha, hb = (json.load(open(os.path.join(d, "hashes.json"))) for d in (dir_a, dir_b))
    bad = 0
    for name in sorted(set(ha) | set(hb)):
        if name not in ha or name not in hb:
            print(f"{name}: only in one run")
            bad += 1
            continue
        la, lb = (open(os.path.join(d, name + ".jsonl")).read().split("\n") for d in (dir_a, dir_b))
        first = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), None if len(la) == len(lb) else min(len(la), len(lb)))
        same_hash = ha[name] == hb[name]
        ok = first is None and (same_hash or name in trace_only)
        bad += not ok
        print(f"{name}: trace {'identical' if first is None else f'DIFFERS at line {first + 1}'} ({len(la) - 2} / {len(lb) - 2} calls), "
              f"hashes {'equal' if same_hash else 'DIFFER'}{' (trace only)' if name in trace_only else ''}")
        if first is not None:
            print("   a:", la[first][:600] if first < len(la) else "<end>")
            print("   b:", lb[first][:600] if first < len(lb) else "<end>")
        if not same_hash:
            print("   differing:", [k for k in ha[name] if ha[name][k] != hb[name].get(k)])
    print("RESULT:", "identical" if bad == 0 else f"{bad} configuration(s) differ")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "--compare":
        rest = sys.argv[4:]
        sys.exit(compare(sys.argv[2], sys.argv[3], set(rest[1:]) if rest and rest[0] == "--trace-only" else set()))
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    record(sys.argv[1], sys.argv[2:])
