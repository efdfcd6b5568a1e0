"""Every allocating wrapper of ops.py, the training step and inference on poisoned, guarded memory (tests/poison.py).

Each case of tests/unwritten_cases.py runs three times on identical guarded inputs — plain, under poisoned(NaN, 0) and
under poisoned(1e30, 1) — and every tensor it returns must have the same BYTES in the three runs, with no guard
touched: an output element that is never written, or a workspace row that is read before it is written, takes the
poison's value in one of the runs (the caching allocator would have handed back the previous, correct, answer).  The
model tests do the same with whole passes of ``UNetHIP`` (fresh allocations), and run a small pass on an engine whose
grow-only scratch buffers (``EngineCore._buf``) a larger pass has left behind, overwritten with poison (stale tails).
The last test holds the allocation sites reached against an ast scan of the product code.

Graph-captured passes are out of scope (the harness raises when an allocation happens during capture).  A HIP error
ends the module: nothing more is started on a device that has faulted.

A guide to a failure: ``PoisonError`` names the result, the first differing element and the allocation site; fix the
kernel or the wrapper (write the missing rows, bound the loop, zero what is accumulated into), not the case."""
import os
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import poison  # noqa: E402
import unwritten_cases as uc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = uc.ROOT
T0 = time.time()
COUNTS = {"cases": 0, "model runs": 0}

uc.add_variant_cases()


def _guard_the_device(fn, *a, **k):
    """run ``fn``; a HIP error (a fault is sticky: every later call would fail or hang) ends the whole session"""
    try:
        return fn(*a, **k)
    except RuntimeError as e:
        text = str(e)
        if any(s in text for s in ("HIP error", "hipError", "illegal memory access", "device-side assert")):
            pytest.exit(f"GPU fault, nothing more is run on this device: {text[:500]}", returncode=3)
        raise


@pytest.mark.parametrize("case", uc.CASES, ids=[c.name for c in uc.CASES])
def test_wrapper_on_poisoned_memory(case):
    COUNTS["cases"] += 1
    flat = _guard_the_device(poison.run_three, case.make, case.call, cut=case.cut, wide_u8=case.wide_u8, ref=case.ref)
    assert flat, "the case returned nothing to compare"
    torch.cuda.synchronize()


def test_the_harness_on_device_memory():
    """what tests/test_poison_host.py shows on the host, once on the device: the poison is in device allocations, an
    element left unset and a store past the end (inside the harness's own buffer: no fault) are both caught"""
    def unset(x):
        out = torch.empty_like(x)
        out[:-1] = 2 * x[:-1]
        if not poison._active:
            out[-1] = 2 * x[-1]
        return out

    def past(x):
        out = torch.empty_like(x)
        out.copy_(2 * x)
        out.as_strided((1,), (1,), out.storage_offset() + out.numel()).fill_(3.0)
        return out
    x = lambda: (torch.arange(1, 12, dtype=torch.float32, device=DEV),)
    with poison.poisoned(poison.NAN, 0):
        assert bool(torch.isnan(torch.empty(5, device=DEV)).all()) and int(torch.empty(5, dtype=torch.int32, device=DEV).sum()) == 0
    with poison.poisoned(poison.SENTINEL, 1):
        assert bool((torch.empty(5, device=DEV, dtype=torch.bfloat16).float() > 9e29).all())
        assert int(torch.empty(5, dtype=torch.uint8, device=DEV).sum()) == 5
    with pytest.raises(poison.PoisonError, match="flat index 10"):
        poison.run_three(x, unset)
    with pytest.raises(poison.GuardError, match="behind the buffer"):
        with poison.poisoned(poison.NAN, 0):
            past(*x())


def test_allocation_during_graph_capture_raises():
    """graph capture is out of scope: an allocation through the harness while the stream captures is refused before
    anything is allocated or launched (the capture itself records nothing and is never replayed)"""
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with poison.poisoned(poison.NAN, 0) as state:
        before = len(state.records)
        with pytest.raises(RuntimeError, match="while a HIP graph is captured"):
            with torch.cuda.graph(graph, stream=side):
                torch.empty(4, device=DEV)
        assert len(state.records) == before
        assert not torch.cuda.is_current_stream_capturing()
        assert bool(torch.isnan(torch.empty(4, device=DEV)).all())          # the block goes on working after the refusal
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------ the model
def _model(kind):
    from deadtrees_amd.network.unet import UNetHIP
    m = UNetHIP(in_channels=3, classes=2, decoder=kind)
    m.reset_parameters(seed=0)
    return m.to(DEV).train()


def _batch(B, H, W, seed=4321):
    from deadtrees_amd.data.synthetic import synth_batch
    img, mask = synth_batch(B, H, W, 3, 2, seed=seed)
    return img.to(DEV), mask.to(DEV)


def _training_pass(m, img, mask, precision):
    """forward + seg_loss + backward through autograd (no optimiser: a fresh model can repeat it) -> what it produced"""
    from deadtrees_amd.loss.seg_loss import seg_loss
    m.train()
    m.precision = precision
    m.zero_grad(set_to_none=True)
    logits = m(img)
    loss, parts, err = seg_loss(logits, mask, None, ("GDICE", "FOCAL"))
    loss.backward()
    torch.cuda.synchronize()
    return dict(logits=logits.detach().clone(), loss=loss.detach().clone(), err=err.clone(), grads=m.smp_grad_dict(),
                bn_state=m.bn_state.detach().clone())


def _inference_pass(m, img, mask, precision):
    out = dict(logits=m.predict_logits(img, precision=precision).clone(), classes=m.predict_classes(img, precision=precision).clone(),
               classes_u8=m.predict_classes(img, dtype="uint8", precision=precision).clone())
    head = m.engine.forward_eval_head if precision == "fp32" else m.engine.forward_bf16_eval_head
    acc, counts, am, err = head(img, m.flat_params.detach(), m.bn_state, mask, want_argmax=True)
    out.update(head_acc=acc.clone(), head_counts=counts.clone(), head_argmax=am.clone(), head_err=err.clone())
    torch.cuda.synchronize()
    return out


def _fresh_passes(img, mask, kind, precision):
    """everything on fresh allocations: a new model, one trainer step (forward, loss, backward, clip, Adam), a training
    pass through autograd, the three inference entry points"""
    from deadtrees_amd.trainer import HipTrainer
    m = _model(kind)
    tr = HipTrainer(m, precision=precision)
    loss = tr.step(img, mask)
    torch.cuda.synchronize()
    step = dict(loss=loss.clone(), err=tr.last["label_error"].clone(), skipped=tr.last["skipped"].clone(),
                grad_norm=tr.last["grad_norm"].clone(), grads=m.smp_grad_dict(), bn_state=m.bn_state.detach().clone(),
                flat_params=m.flat_params.detach().clone())
    COUNTS["model runs"] += 1
    return step, _training_pass(m, img, mask, precision), _inference_pass(m.eval(), img, mask, precision)


MODEL_CASES = [(kind, precision, (2, 64, 96)) for kind in ("unet", "resunet", "unetplusplus") for precision in ("fp32", "bf16")]
MODEL_CASES.append(("unet", "fp32", (2, 128, 128)))      # whole Winograd tiles at the upper levels: the FULL epilogue forms


@pytest.mark.parametrize("kind,precision,shape", MODEL_CASES, ids=[f"{k}-{p}-{s[1]}x{s[2]}" for k, p, s in MODEL_CASES])
def test_model_passes_on_fresh_poisoned_allocations(kind, precision, shape):
    flat = _guard_the_device(poison.run_three, lambda: _batch(*shape),
                             lambda img, mask: _fresh_passes(img, mask, kind, precision))
    names = [p for p, _ in flat]
    assert any("flat_params" in p for p in names) and any("head_acc" in p for p in names)


@pytest.mark.parametrize("K,H,W", [(2, 37, 61), (3, 16, 20)])
def test_loss_variants_on_poisoned_memory(K, H, W):
    """the options of loss/seg_loss.py the training passes above do not take: the generalised Wasserstein dice term (its
    position sums and their gradient), the boundary term with distance maps, the probabilities of loss_sums"""
    def make():
        g = torch.Generator().manual_seed(K + H)
        labels = torch.randint(0, K, (2, H, W), generator=g).to(DEV)
        from deadtrees_amd import ops
        return dict(logits=(2 * torch.randn((2, K, H, W), generator=g)).to(DEV), labels=labels, dist=ops.signed_distmap(labels, K)[0])

    def call(logits, labels, dist):
        from deadtrees_amd.loss.seg_loss import loss_sums, seg_loss
        x = logits.clone().requires_grad_(True)
        loss, parts, err = seg_loss(x, labels, dist, ("GWDICE", "FOCAL", "BOUNDARY"))
        loss.backward()
        return loss.detach(), {k: v.detach() for k, v in parts.items()}, err, x.grad, loss_sums(logits, labels, dist, want_probs=True)
    _guard_the_device(poison.run_three, make, call)


def test_efficientunetplusplus_inference_on_fresh_poisoned_allocations():
    """the inference-only decoder (pointwise / depthwise / scSE kernels of csrc/mbconv.hip) at 2 x 64 x 96"""
    def passes(img, mask):
        from deadtrees_amd.network.unet import UNetHIP
        m = UNetHIP(in_channels=3, classes=2, decoder="efficientunetplusplus")
        m.reset_parameters(seed=0)
        m = m.to(DEV).eval()
        COUNTS["model runs"] += 1
        with torch.no_grad():
            return m(img).clone(), m.predict_logits(img).clone(), m.predict_classes(img, dtype="uint8").clone()
    _guard_the_device(poison.run_three, lambda: _batch(2, 64, 96), passes)


# entries of EngineCore._ws that are state, not scratch: a cache with a key.  They are left alone by the stale-tail test
STATE_ENTRIES = {
    "_key": "the key of a cache: compared on the host before the cached image is used",
    "wino_u_val": "the Winograd weight images of the current parameters, rebuilt when wino_u_key changes",
    "const_": "a vector of one constant, filled when it is made (torch.full)",
    "side_stream": "a stream, not a tensor",
}


def _is_state(name, engine_ws):
    return any(tag in name for tag in STATE_ENTRIES) or (name + "_key") in engine_ws


def _poison_scratch(m, handed_out, value):
    """overwrite every scratch buffer ``EngineCore._buf`` has handed out so far: floats with ``value``, integers with
    0 (value NaN) or 1; -> the names overwritten, the names left alone as state"""
    ws = m.engine._ws
    hit, kept = [], []
    torch.cuda.synchronize()
    for name in sorted(ws):
        t = ws[name]
        if not isinstance(t, torch.Tensor) or name not in handed_out or _is_state(name, ws):
            kept.append(name)
            continue
        if t.dtype.is_floating_point:
            t.fill_(value)
        else:
            t.view(torch.uint8).zero_()
            if value == value:
                t.view(torch.uint8)[::t.element_size()] = 1
        hit.append(name)
    if m._grads is not None:          # the flat gradient buffer is an output of the backward pass: every element written
        m._grads.fill_(value)
    return hit, kept


@pytest.fixture
def recorded_buffers():
    """wrap EngineCore._buf for the length of a test: the names it hands out"""
    from deadtrees_amd.network.engine_core import EngineCore
    names, orig = set(), EngineCore._buf

    def _buf(self, name, *a, **k):
        names.add(name)
        return orig(self, name, *a, **k)
    EngineCore._buf = _buf
    try:
        yield names
    finally:
        EngineCore._buf = orig


def _fresh_copy(m, kind):
    f = _model(kind)
    with torch.no_grad():
        f.flat_params.data.copy_(m.flat_params.data)
        f.bn_state.copy_(m.bn_state)
    return f


def _same(a, b, what):
    fa, fb = list(poison.flatten(a)), list(poison.flatten(b))
    assert [p for p, _ in fa] == [p for p, _ in fb], what
    for (p, x), (_, y) in zip(fa, fb):
        assert poison.same_bytes(x, y), f"{what}: {p}: {poison._first_difference(x, y)}"


SEQUENCES = {      # (first pass at 2 x 96 x 128, [passes at 2 x 64 x 96 ...]): (mode, precision)
    "train, train": (("train", "fp32"), [("train", "fp32")]),
    "train, inference, train": (("train", "fp32"), [("infer", "fp32"), ("train", "fp32")]),
    "bf16 train, fp32 train": (("train", "bf16"), [("train", "fp32")]),
    "fp32 train, bf16 inference, bf16 train": (("train", "fp32"), [("infer", "bf16"), ("train", "bf16")]),
    "inference, train": (("infer", "fp32"), [("train", "bf16")]),
}


@pytest.mark.parametrize("kind", ["unet", "resunet", "unetplusplus"])
@pytest.mark.parametrize("sequence", list(SEQUENCES))
def test_small_pass_after_a_large_one_reads_no_stale_tail(kind, sequence, recorded_buffers):
    first, later = SEQUENCES[sequence]
    big, small = _batch(2, 96, 128, seed=11), _batch(2, 64, 96, seed=12)
    run = {"train": _training_pass, "infer": _inference_pass}

    def body():
        m = _model(kind)
        run[first[0]](m if first[0] == "train" else m.eval(), *big, first[1])
        for value in (poison.NAN, poison.SENTINEL):
            for mode, precision in later:
                hit, kept = _poison_scratch(m, recorded_buffers, value)
                assert hit, "no scratch buffer was recorded: EngineCore._buf is not what hands them out any more"
                assert all(_is_state(n, m.engine._ws) or n not in recorded_buffers for n in kept)
                f = _fresh_copy(m, kind)
                got = run[mode](m if mode == "train" else m.eval(), *small, precision)
                want = run[mode](f if mode == "train" else f.eval(), *small, precision)
                _same(got, want, f"{kind}, {sequence}: {mode} {precision} after scratch := {value}")
                for p, t in poison.flatten(got):
                    assert not t.dtype.is_floating_point or bool(torch.isfinite(t).all()), (p, sequence)
    _guard_the_device(body)
    COUNTS["model runs"] += 1


# ------------------------------------------------------------------------------------------------------ coverage
SCANNED = ["deadtrees_amd/ops.py", "deadtrees_amd/network/module.py", "deadtrees_amd/loss/seg_loss.py",
           "deadtrees_amd/data/pool.py", "deadtrees_amd/data/rasters.py"]
# allocation sites outside ops.py that the passes above do not reach: "file:function" -> (how many sites of that function
# are excused, the option that guards them).  The count is held: a torch.empty added to a listed function is looked at
DATA = ("fills device pools from shard / raster files (uploads and raster_cut write them); the kernels behind them run in the "
        "pool_gather_* and raster_cut cases, the loaders in tests/test_pool_gpu.py and tests/test_rasters_gpu.py")
NOT_REACHED = {
    "deadtrees_amd/network/module.py:patch_first_conv": (1, "host tensor of a pretrained first convolution for in_channels != 3 "
                                                        "(load_pretrained_encoder); every channel is written by the loop below it"),
    "deadtrees_amd/network/module.py:UNetHIP.init_decoder_smp": (1, "host tensors handed to nn.init (decoder initialisation next to a "
                                                                "pretrained encoder)"),
    "deadtrees_amd/network/engine_core.py:EngineCore._bf16_weights": (1, "the miss path of ONE bf16 weight image; the engine builds the "
                                                                     "four images together, so its passes find the cache filled"),
    "deadtrees_amd/data/pool.py:DevicePool.__init__.alloc": (1, "pinned host staging (pin_memory=True) of a pool on a device: " + DATA),
    "deadtrees_amd/data/pool.py:DevicePool.__init__": (4, "DevicePool(device=...): " + DATA),
    "deadtrees_amd/data/pool.py:combined_plan": (4, "host index tables of an epoch, every column assigned by the loop below them"),
    "deadtrees_amd/data/pool.py:_GatherLoader.__iter__": (1, "the lu tensor next to HipTrainer.static_batch() (graph replay: out of "
                                                             "scope); pool_gather_combined with out= is a case"),
    "deadtrees_amd/data/rasters.py:_DeviceRows._alloc": (4, "pool_from_rasters(device=...): " + DATA),
    "deadtrees_amd/data/rasters.py:pool_from_rasters": (3, "pool_from_rasters(device=...): " + DATA),
}


def test_allocation_sites_were_reached():
    """the union of the sites recorded above against the ast scan.  Meaningful only when the whole module has run"""
    import glob
    if COUNTS["cases"] < len(uc.CASES):
        pytest.skip("a partial run of the module (-k): the site coverage needs every case of the table")
    files = SCANNED + sorted(os.path.relpath(p, ROOT) for p in glob.glob(os.path.join(ROOT, "deadtrees_amd", "network", "engine_*.py")))
    missing_ops, missing_other, listed, used = [], [], [], {}
    total = 0
    for rel in files:
        for line, top, fn in uc.allocation_sites(os.path.join(ROOT, rel)):
            total += 1
            if f"{rel}:{line}" in poison.reached:
                continue
            if rel.endswith("ops.py"):
                missing_ops.append(f"{rel}:{line} ({top}: torch.{fn})")
            elif f"{rel}:{top}" in NOT_REACHED:
                listed.append(f"{rel}:{line} ({top}): {NOT_REACHED[f'{rel}:{top}'][1]}")
                used[f"{rel}:{top}"] = used.get(f"{rel}:{top}", 0) + 1
            else:
                missing_other.append(f"{rel}:{line} ({top}: torch.{fn})")
    print(f"\n[unwritten] {COUNTS['cases']} wrapper cases, {COUNTS['model runs']} model runs, "
          f"{total - len(listed) - len(missing_ops) - len(missing_other)} of the {total} torch.empty* sites scanned in {len(files)} "
          f"files reached ({len(poison.reached)} sites with torch.zeros / torch.full and other modules), {poison.stats['buffers']} guarded buffers "
          f"({poison.stats['bytes'] / 2 ** 20:.0f} MiB), {time.time() - T0:.0f} s since the module was imported")
    print("[unwritten] sites not reached, by the option that guards them:\n  " + "\n  ".join(listed or ["(none)"]))
    print("[unwritten] NOT reached and not listed:\n  " + "\n  ".join(missing_ops + missing_other or ["(none)"]))
    assert not missing_ops, "ops.py allocation sites no case reaches:\n  " + "\n  ".join(missing_ops)
    assert used == {k: v[0] for k, v in NOT_REACHED.items()}, f"sites not reached per listed function {used} against the list"
    assert not missing_other, "allocation sites neither reached nor listed in NOT_REACHED:\n  " + "\n  ".join(missing_other)
