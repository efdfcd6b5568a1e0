"""The case generator of the convolution variant tests (tests/conv_variant_cases.py) names exactly the variants the recorded
dispatch table names (tests/golden/dispatch_table.json, network rows): a new dispatch branch that gets a table row and no
numerical case fails here.  Host only: the keys come from the library's config queries, no GPU needed."""
import pytest

import conv_variant_cases as cvc


def _cases():
    import __graft_entry__ as g
    g.build()
    return cvc.cases()


def _assert_covers(prec, got, keys):
    """every key of the table has a case.  (The other direction cannot fail here: cases() keeps table keys only, and
    whether every key of the library has a table row is the business of tests/test_dispatch_table.py)"""
    assert not keys - got, f"{prec} variants of the table without a case: {sorted(keys - got)}"


def test_generated_keys_equal_the_keys_of_the_dispatch_table():
    cases = _cases()
    f32, bf = cvc.golden_keys()
    assert len(f32) == 78 and len(bf) == 77                  # the counts the table gave when this test was written
    for prec, keys, keyf in (("fp32", f32, cvc.fp32_key), ("bf16", bf, cvc.bf16_key)):
        _assert_covers(prec, set(cases[prec]), keys)
        for key, t in cases[prec].items():
            assert keyf(t) == key, (prec, key, t)            # every descriptor dispatches to the key it stands for
    for key, t in cases["bf16_extra"].items():
        assert key not in bf and cvc.bf16_key(t) == key
    assert set(cases["bf16_extra"]) == set(cvc.EXTRA_BF16_KEYS)
    for prec, keys in (("fp32", f32), ("bf16", bf)):
        off = cases["off_table"][prec]
        print(f"{prec}: the search met {len(off)} variant keys that no network row of the table has (no case generated)")
        assert not set(off) & keys


def test_a_key_missing_from_the_generator_is_noticed():
    """the comparison of the first test, on a generator output with one key taken out"""
    cases = _cases()
    f32, _ = cvc.golden_keys()
    for key in sorted(cases["fp32"])[::7]:
        with pytest.raises(AssertionError, match="without a case"):
            _assert_covers("fp32", set(cases["fp32"]) - {key}, f32)


def test_generated_descriptors_are_within_budget():
    cases = _cases()
    for prec in ("fp32", "bf16", "bf16_extra"):
        for key, t in cases[prec].items():
            assert cvc.macs(t) <= cvc.MAX_MACS, (prec, key, t, cvc.macs(t))
            assert cvc.largest_tensor_bytes(t) < cvc.MAX_TENSOR_BYTES, (prec, key, t)
            assert cvc.within_budget(t)


def test_generation_is_deterministic():
    first = _cases()
    cvc.cases.cache_clear()
    assert cvc.cases() == first


def test_the_wide_and_the_special_variants_are_there():
    cases = _cases()
    f32 = [dict(zip(cvc.FP32_KEY, k)) for k in cases["fp32"]]
    bf = [dict(zip(cvc.BF16_KEY, k)) for k in cases["bf16"]]

    def has(rows, **want):
        return any(all(r[n] == v for n, v in want.items()) for r in rows)

    # the two zero-insertion instantiations at 64 output channels per workgroup: launch<3,1,32,64,16,true>, <1,1,...>
    assert has(f32, ksize=3, stride=1, mode0=2, tw=32, tn=64, ck=16, uses_zi=1)
    assert has(f32, ksize=1, stride=1, mode0=2, tw=32, tn=64, ck=16, uses_zi=1)
    for tw in (8, 16, 32):
        assert has(f32, tn=64, tw=tw, ksize=3, stride=1, uses_zi=0)
        assert has(f32, tn=64, tw=tw, ksize=1, stride=1, uses_zi=0)
    for tw in (8, 16):
        assert has(bf, tn=64, tw=tw, mt=2, ksize=3)
    assert has(bf, mt=8)
    assert has(bf, mt=8, mode0=2) and has(bf, mt=8, concat=1) and has(bf, mt=8, split=1) and has(bf, mt=8, accumulate=1)
    # a 64-wide case needs its batch: every one of them has a single-image twin on a 32-wide (or narrower) kernel
    for prec, cfg in (("fp32", cvc.fp32_config), ("bf16", cvc.bf16_config)):
        for key, t in cases[prec].items():
            if key[4] == 64 and t[0] > 1:
                assert cfg((1,) + tuple(t[1:]))[1] < 64, (prec, key, t)


def test_a_non_finite_device_result_fails_the_output_and_statistics_checks():
    """the comparison helpers of tests/test_conv_variants_gpu.py on the host: one NaN or inf among correct values gives an
    infinite ratio and so a failure (Python's max(0.0, nan) is 0.0: a NaN must not get lost on the way), for a plain, a
    split, a joined and a lean-kernel case, in the outputs and in the per-image and the whole-batch statistics"""
    import math

    import torch

    import test_conv_variants_gpu as tv
    _cases()
    for prec, key_filter in (("fp32", lambda k: k[8] == 0 and k[9] == 0), ("fp32", lambda k: k[8] == 1),
                             ("bf16", lambda k: k[9] == 1), ("fp32", lambda k: k[5] >= 1000)):
        key = next(k for k in sorted(cvc.cases()[prec]) if key_filter(k) and k[2] == 0 and k[4] <= 32)
        t = cvc.cases()[prec][key]
        d = dict(zip(cvc.FIELDS, t))
        inp = tv._inputs(t, prec, seed=1)
        want, mag = tv._reference(t, inp)
        exact = [p[0].permute(0, 2, 3, 1).contiguous().float() for p in tv._parts(t, inp, want, mag)] + [None]
        assert tv._check_outputs(t, prec, inp, exact[:2], want, mag) <= 1.0
        for bad in (math.nan, math.inf):
            for which in range(2 if d["cout_split"] else 1):
                outs = [None if o is None else o.clone() for o in exact[:2]]
                outs[which][0, 0, 0, -1] = bad
                assert tv._check_outputs(t, prec, inp, outs, want, mag) == math.inf
        if not d["cout_split"] and not d["accumulate"]:
            B, C = d["B"], d["Cout"]
            tiles = next((k for k in range(1, 65) if tv._rows_per_image(prec, t, B * k)), 0)     # 0: a persistent kernel
            P = B * tiles if tiles else 5
            total = torch.stack([want.sum(dim=(2, 3)), (want * want).sum(dim=(2, 3))])           # [2, B, C]
            rows = (total[:, :, None, :] / tiles).expand(2, B, tiles, C).reshape(2, P, C) if tiles else \
                (total.sum(dim=1, keepdim=True) / P).expand(2, P, C)
            rows = rows.float().contiguous()
            assert max(tv._check_stats(prec, t, rows, want, mag)) <= 1.0
            for bad in (math.nan, math.inf):
                for which in (0, 1):
                    broken = rows.clone()
                    broken[which, P - 1, 0] = bad
                    assert tv._check_stats(prec, t, broken, want, mag)[which] == math.inf
