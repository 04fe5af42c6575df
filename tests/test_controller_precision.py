"""CPU checks of the reference-precision controller form (AcConfig.controller_precision = AC_CTL_FP32): the three-bf16-piece split the
weights and activations go through (ac_split_bf16x3 meets the bound include/aircombat.h states), the config field's default, and the
Python surface refusing an unknown form before any GPU is touched."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bf16_rne(x):
    """float32 -> the nearest bf16 (ties to even), returned as float32."""
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return r.astype(np.uint32).view(np.float32)


def _split(lib, x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    b = [np.empty_like(x) for _ in range(3)]
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.dll.ac_split_bf16x3(p(x), x.size, p(b[0]), p(b[1]), p(b[2])) == 0, lib.last_error()
    return b


def test_split_bf16x3_bound(pkg):
    lib = pkg.load_library()
    rng = np.random.default_rng(11)
    # random significands over binades 2^-103 .. 2^127 (the range the bound is stated for), both signs
    e = rng.uniform(-103.0, 127.0, size=200_000)
    x = (np.sign(rng.standard_normal(e.size)) * np.exp2(e)).astype(np.float32)
    special = np.array([0.0, -0.0, 1e-30, -1e-30, 2.0 ** -103, -(2.0 ** -103), 1e38, -1e38, 3.3e38, -3.3e38, 1.0, -1.0,
                        1.0 / 3.0, -2.0 / 3.0, 0.1, -7.25, 65504.0, np.float32(np.pi)], dtype=np.float32)
    x = np.concatenate([x, special])
    b0, b1, b2 = _split(lib, x)
    for piece in (b0, b1, b2):
        assert np.isfinite(piece).all()
        assert (piece.view(np.uint32) & 0xFFFF == 0).all()        # exactly bf16-representable
    assert (b0 == _bf16_rne(x)).all()                              # round to nearest even
    assert (b1 == _bf16_rne(x - b0)).all()
    f = lambda a: a.astype(np.float64)
    left = np.abs(f(x) - f(b0) - f(b1) - f(b2))
    assert (left <= 2.0 ** -24 * np.abs(f(x))).all(), left.max()
    assert (left == 0.0).all()                                     # (in that range the split is in fact exact)
    z = slice(x.size - special.size, x.size - special.size + 2)   # 0 and -0 split into zeros
    assert (b0[z] == 0).all() and (b1[z] == 0).all() and (b2[z] == 0).all()
    # below 2^-103 the stated bound is absolute
    t = (np.exp2(rng.uniform(-126.0, -103.0, size=10_000)) * np.sign(rng.standard_normal(10_000))).astype(np.float32)
    c0, c1, c2 = _split(lib, t)
    assert (np.abs(f(t) - f(c0) - f(c1) - f(c2)) < 2.0 ** -126).all()


def test_split_bf16x3_products_beat_fp32_rounding(pkg):
    """The six kept terms of a product (i + j <= 2) are within about 2^-23 of it: at least fp32's own rounding of the product."""
    lib = pkg.load_library()
    rng = np.random.default_rng(12)
    x = rng.standard_normal(100_000).astype(np.float32)
    y = rng.standard_normal(100_000).astype(np.float32)
    a, b = _split(lib, x), _split(lib, y)
    f = lambda v: v.astype(np.float64)
    kept = sum(f(a[i]) * f(b[j]) for i in range(3) for j in range(3) if i + j <= 2)
    exact = f(x) * f(y)
    rel = np.abs(kept - exact) / np.abs(exact)
    assert rel.max() <= 2.0 ** -23, rel.max()


def test_controller_precision_defaults_to_fast(pkg):
    assert pkg.capi.AC_CTL_FAST == 0 and pkg.capi.AC_CTL_FP32 == 1
    for task in ("singlecombat", "hierarchical_singlecombat", "scenario1"):
        assert pkg.default_config(task).controller_precision == 0
    assert pkg.default_nvn_config(2, hierarchical=True).controller_precision == 0
    cfg_dir = os.path.join(ROOT, "aircombat-selfplay_amd", "data")
    yamls = [os.path.join(dp, f) for dp, _, fs in os.walk(cfg_dir) for f in fs if f.endswith(".yaml")]
    for y in yamls[:20]:
        try:
            cfg = pkg.config_from_yaml(y)
        except (NotImplementedError, ValueError, KeyError):
            continue
        assert cfg.controller_precision == 0, y


def test_unknown_controller_precision_is_refused_before_the_gpu(pkg):
    cfg = pkg.default_config("hierarchical_singlecombat")

    class NoLib:   # any call into the library would fail the test: the keyword is checked first
        def __getattr__(self, name):
            raise AssertionError(f"library touched: {name}")

    with pytest.raises(ValueError, match="controller_precision"):
        pkg.HipVecEnv(cfg, 2, controller_precision="bogus", lib=NoLib())
    with pytest.raises(ValueError, match="controller_precision"):
        pkg.HipShareVecEnv(pkg.default_nvn_config(2, hierarchical=True), 2, controller_precision="fp64", lib=NoLib())
    with pytest.raises(ValueError):
        pkg.controller_forward(np.zeros(12), np.zeros(128), precision="half")
    assert cfg.controller_precision == 0   # the caller's config is not modified
