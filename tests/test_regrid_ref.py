"""Regridding, host side: the numpy restatement tests/regrid_ref.py against scipy.ndimage, csrc/regrid_core.h
compiled with g++ (plain and under the address / undefined-behaviour sanitizers, as a stand-alone program) against the
restatement, the index-matrix algebra and the argument checks of the new entry points.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch
from scipy import ndimage

from tests import regrid_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ENTRY_POINTS = ("mi355_bspline_prefilter", "mi355_regrid")
_ID = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)        # noqa: E731


# ------------------------------------------------------------------------------------------------ the cases themselves
@pytest.mark.parametrize("src,dst,name", R.CASES + R.EXACT_CASES, ids=_ID)
def test_cases_are_not_vacuous_and_leave_out_little(src, dst, name):
    """at least 0.14 of a case's voxels are inside; at most 1 % lie within the tolerance of an inside boundary"""
    k = R.case(src, dst, name)
    print(f"{src}->{dst} {name}: inside {k['inside'].mean():.3f}, boundary {k['boundary'].mean():.4f}, tie {k['tie'].mean():.4f}")
    assert k["inside"].mean() >= 0.14
    assert k["boundary"].mean() <= 0.01
    if (src, dst, name) in R.NEAREST_CASES + R.EXACT_CASES:
        assert k["tie"].mean() == 0.0


def test_exact_fma_of_the_coordinates():
    """the rational fma rounds once: a case where round(round(a b) + c) differs from round(a b + c)"""
    a, b, c = 1.0 + 2.0 ** -30, 2 ** 30 + 1, -float(2 ** 30 + 2)
    got = R._fma(a, np.array([b]), np.array([c]))[0]
    assert got == 2.0 ** -30 and a * b + c != got


# ------------------------------------------------------------------------------------------------ restatement vs scipy
@pytest.mark.parametrize("src", [s for s, _ in R.PAIRS], ids=_ID)
def test_prefilter_against_scipy(src):
    x = R.volume(3, src)
    want = np.stack([ndimage.spline_filter(ch.astype(np.float64), order=3, mode="mirror", output=np.float64) for ch in x])
    err, bound = np.abs(R.prefilter(x) - want).max(), R.coefficient_bound(np.abs(x).max())
    print(f"prefilter {src}: max |restatement - scipy| = {err:.3e} (bound {bound:.3e}), max |coefficient| = {np.abs(want).max():.2f}")
    assert err <= bound


def _scipy(k, order, dst):
    mode = "mirror" if order == 3 else "nearest"
    return np.stack([ndimage.affine_transform(ch.astype(np.float64), k["m"][:, :3], k["m"][:, 3], dst, order=order, mode=mode,
                                              output=np.float64) for ch in k["x"]])


@pytest.mark.parametrize("order", [1, 3])
@pytest.mark.parametrize("src,dst,name", R.CASES + R.EXACT_CASES, ids=_ID)
def test_interpolation_against_scipy(src, dst, name, order):
    """inside voxels of orders 1 (mode='nearest') and 3 (mode='mirror'), within 64 f64 ulps of 27 max|x|"""
    k = R.case(src, dst, name)
    keep = k["inside"] & ~k["boundary"]
    err, bound = np.abs(k[order] - _scipy(k, order, dst))[:, keep].max(), R.coefficient_bound(k["xmax"])
    print(f"order {order} {src}->{dst} {name}: max |restatement - scipy| = {err:.3e} (bound {bound:.3e})")
    assert err <= bound


@pytest.mark.parametrize("src,dst,name", R.NEAREST_CASES + R.EXACT_CASES, ids=_ID)
def test_nearest_against_scipy(src, dst, name):
    k = R.case(src, dst, name)
    keep = k["inside"] & ~k["boundary"] & ~k["tie"]
    np.testing.assert_array_equal(k[0][:, keep], _scipy(k, 0, dst)[:, keep])


def test_exact_cases_return_the_samples():
    """identity and integer translation: order 0 and 1 return the gathered input exactly, order 3 within the bound (the
    prefilter inverts the sampling); outside voxels hold the fill"""
    for src, dst, name in R.EXACT_CASES:
        k = R.case(src, dst, name)
        shift = (0, 0, 0) if name == "identity" else R.SHIFT
        idx = np.meshgrid(*[np.arange(n) + t for n, t in zip(src, shift)], indexing="ij")
        ins = np.all([(i >= 0) & (i < n) for i, n in zip(idx, src)], axis=0)
        np.testing.assert_array_equal(ins, k["inside"])
        want = np.where(ins, k["x"].astype(np.float64)[(slice(None),) + tuple(np.clip(i, 0, n - 1) for i, n in zip(idx, src))], 0.0)
        np.testing.assert_array_equal(k[0], want)
        np.testing.assert_array_equal(k[1], want)
        assert np.abs(k[3] - want).max() <= R.coefficient_bound(k["xmax"])
        got = R.regrid(k["x"], k["m"], dst, 1, -1.5, k["s"])[0]
        assert np.all(got[:, ~ins] == -1.5) and np.array_equal(got[:, ins], want[:, ins])


# ---------------------------------------------------------------------------------------------- core header on the host
def _build(tmp_path, name, flags):
    exe = tmp_path / name
    subprocess.check_call(["g++", "-O2", *flags, "-o", str(exe), os.path.join(HERE, "host_regrid_check.cpp"), "-lm"])
    return exe


def _run_host(exe, tmp_path, k, dst, order, fill):
    x = k["x"].astype(np.float64)
    head = [x.shape[0], *x.shape[1:], *dst, order, fill, *k["m"].reshape(-1)]
    np.concatenate([np.asarray(head, np.float64), x.ravel()]).tofile(tmp_path / "in.bin")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1")
    subprocess.check_call([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], env=env)
    o = np.fromfile(tmp_path / "out.bin")
    return o[:x.size].reshape(x.shape), o[x.size:].reshape((x.shape[0],) + tuple(dst))


def _check_host(exe, tmp_path):
    worst = 0.0
    for src, dst in R.PAIRS[1:3]:
        for name in R.MATRICES:
            k = R.case(src, dst, name)
            bound = R.coefficient_bound(k["xmax"])
            for order in (0, 1, 3):
                for fill in R.FILLS:
                    coef, got = _run_host(exe, tmp_path, k, dst, order, fill)
                    want = np.where(k["inside"], k[order], fill)
                    keep = ~(k["boundary"] | k["tie"]) if order == 0 else ~k["boundary"]
                    assert np.all(got[:, ~k["inside"] & keep] == fill)
                    worst = max(worst, np.abs(got - want)[:, keep].max() / bound)
                    if order == 3:
                        worst = max(worst, np.abs(coef - k["coef"]).max() / bound)
                    assert worst <= 1.0
    return worst


def test_core_arithmetic_on_host_matches_restatement(tmp_path):
    """csrc/regrid_core.h is plain C++: the SAME prefilter, coordinates, taps and sums the HIP kernels run, compiled with g++"""
    worst = _check_host(_build(tmp_path, "hrg", []), tmp_path)
    print(f"host build: max |core - restatement| / (64 ulps of 27 max|x|) = {worst:.3e}")


def test_core_arithmetic_on_host_under_sanitizers(tmp_path):
    """the same stand-alone program with -fsanitize=address,undefined: a finding aborts it (non-zero exit)"""
    _check_host(_build(tmp_path, "hrg_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]), tmp_path)


# ----------------------------------------------------------------------------------------------------- index matrices
def _affine(rng):
    a = np.eye(4)
    a[:3, :3] = rng.standard_normal((3, 3)) + 2 * np.eye(3)
    a[:3, 3] = rng.uniform(-50, 50, 3)
    return a


def test_index_matrix_algebra():
    from unet_bssfp_amd import preprocess as P
    rng = np.random.default_rng(3)
    a, b, c, x = _affine(rng), _affine(rng), _affine(rng), _affine(rng)
    full = lambda m: np.concatenate([m, [[0, 0, 0, 1.0]]])                      # noqa: E731
    m_ab = P.index_matrix(a, b)
    assert m_ab.shape == (3, 4) and m_ab.dtype == np.float64 and m_ab.flags["C_CONTIGUOUS"]
    np.testing.assert_allclose(m_ab, (np.linalg.inv(a) @ b)[:3], rtol=0, atol=1e-12)
    np.testing.assert_allclose(P.index_matrix(a, b, x), (np.linalg.inv(a) @ x @ b)[:3], rtol=0, atol=1e-10)
    # composition: c -> b -> a is c -> a; inverse: a -> b then b -> a is the identity; the same grid is the identity
    np.testing.assert_allclose(full(m_ab) @ full(P.index_matrix(b, c)), full(P.index_matrix(a, c)), rtol=0, atol=1e-10)
    np.testing.assert_allclose(full(m_ab) @ full(P.index_matrix(b, a)), np.eye(4), rtol=0, atol=1e-10)
    np.testing.assert_allclose(P.index_matrix(a, a), np.eye(4)[:3], rtol=0, atol=1e-12)
    # a world-to-world matrix and its inverse swap the roles of the two grids
    np.testing.assert_allclose(full(P.index_matrix(a, b, x)) @ full(P.index_matrix(b, a, np.linalg.inv(x))), np.eye(4), rtol=0, atol=1e-9)
    # a 1 mm grid and the 2 mm grid over the same field of view: voxel i of the coarse grid covers fine voxels 2 i and 2 i + 1
    fine, coarse = np.eye(4), np.diag([2.0, 2.0, 2.0, 1.0])
    coarse[:3, 3] = 0.5
    np.testing.assert_array_equal(P.index_matrix(fine, coarse), np.concatenate([2 * np.eye(3), np.full((3, 1), 0.5)], 1))
    np.testing.assert_array_equal(P.index_matrix(coarse, fine), np.concatenate([0.5 * np.eye(3), np.full((3, 1), -0.25)], 1))


def test_index_matrix_value_errors():
    from unet_bssfp_amd import preprocess as P
    good = np.diag([2.0, 2.0, 2.0, 1.0])
    flat = good.copy()
    flat[2, :3] = flat[0, :3]
    for bad in (flat, np.zeros((4, 4))):
        with pytest.raises(ValueError, match="singular"):
            P.index_matrix(bad, good)
        with pytest.raises(ValueError, match="singular"):
            P.index_matrix(good, bad)
        with pytest.raises(ValueError, match="singular"):
            P.index_matrix(good, good, bad)
    with pytest.raises(ValueError, match="4 x 4"):
        P.index_matrix(good[:3], good)
    nan = good.copy()
    nan[0, 3] = np.nan
    with pytest.raises(ValueError, match="finite"):
        P.index_matrix(good, nan)


# ---------------------------------------------------------------------------------------------------- argument checks
def test_entry_points_are_declared_built_and_exported():
    from unet_bssfp_amd import _lib
    make = open(os.path.join(ROOT, "unet_bssfp_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bregrid\.hip\b", make, flags=re.M)
    header = open(_lib.HEADER_PATH).read()
    assert "#define MI355_REGRID_MAX_N 512" in header and _lib.H["REGRID_MAX_N"] == 512
    assert (_lib.H["REGRID_NEAREST"], _lib.H["REGRID_LINEAR"], _lib.H["REGRID_CUBIC"]) == (0, 1, 3)
    assert len(_lib._structs) == 12                                          # the feature adds no struct
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)


def test_argument_checks_before_any_launch():
    """bad arguments return MI355_ERR_ARG (an extent over 512: MI355_ERR_UNSUPPORTED) with a message; nothing is launched
    (there is no GPU here, and the pointers are small integers that no kernel could touch)"""
    import ctypes as C
    from unet_bssfp_amd import _lib
    lib, E, U = _lib.load(), _lib.H["ERR_ARG"], _lib.H["ERR_UNSUPPORTED"]
    err = lambda: lib.mi355_last_error()                                  # noqa: E731
    p, far = 4096, 4096 + (1 << 30)
    pre = lambda **k: lib.mi355_bspline_prefilter(*[{**dict(x=p, coef=far, c=2, d=5, h=7, w=9, stream=None), **k}[a]   # noqa: E731
                                                    for a in ("x", "coef", "c", "d", "h", "w", "stream")])
    for k in ("x", "coef"):
        assert pre(**{k: None}) == E and b"null" in err()
    for k in ("d", "h", "w"):
        assert pre(**{k: 0}) == E and b"positive" in err()
        assert pre(**{k: -4}) == E and b"positive" in err()
        assert pre(**{k: 513}) == U and b"exceed 512" in err()
    assert pre(c=0) == E and b"channels" in err()
    assert pre(coef=p + 64) == E and b"overlaps" in err()
    assert pre(c=65536, d=512, h=512) == E and b"rows" in err()
    m = (C.c_double * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
    base = dict(src=p, out=far, c=2, sd=5, sh=7, sw=9, od=4, oh=4, ow=4, m=m, order=1, fill=0.0, stream=None)
    rg = lambda **k: lib.mi355_regrid(*[{**base, **k}[a] for a in base])   # noqa: E731
    for k in ("src", "out", "m"):
        assert rg(**{k: None}) == E and b"null" in err()
    for order in (2, -1, 4):
        assert rg(order=order) == E and b"order" in err()
    for k in ("sd", "sh", "sw"):
        assert rg(**{k: 0}) == E and b"source extents" in err()
    for k in ("od", "oh", "ow"):
        assert rg(**{k: 0}) == E and b"output extents" in err()
        assert rg(**{k: 4097}) == E and b"output extents" in err()
    assert rg(c=0) == E and b"channels" in err()
    assert rg(m=(C.c_double * 12)(*([1.0] * 11 + [float("nan")]))) == E and b"entry 11" in err()
    assert rg(out=p + 16) == E and b"overlaps" in err()


def test_wrappers_raise_on_bad_arguments_and_cpu_tensors():
    from unet_bssfp_amd import _lib, preprocess as P
    x, eye = torch.ones(2, 3, 4, 5), np.eye(4)
    with pytest.raises(ValueError, match="interpolation"):
        P.regrid(x, eye, (3, 4, 5), "cubic")
    with pytest.raises(ValueError, match="matrix"):
        P.regrid(x, np.eye(3), (3, 4, 5))
    with pytest.raises(ValueError, match="matrix"):
        P.regrid(x, np.full((3, 4), np.inf), (3, 4, 5))
    with pytest.raises(ValueError, match="out_shape"):
        P.regrid(x, eye, (3, 4))
    with pytest.raises(ValueError, match="out_shape"):
        P.regrid(x, eye, (3, 0, 5))
    for how in ("nearest", "linear", "bspline"):
        with pytest.raises(_lib.Mi355Error, match="GPU only"):
            P.regrid(x, eye, (3, 4, 5), how)
    with pytest.raises(_lib.Mi355Error, match="GPU only"):
        P.bspline_coefficients(x)
    with pytest.raises(ValueError, match="unknown options"):
        P._regrid_options({"interpolation": "linear", "order": 3})
    with pytest.raises(ValueError, match="interpolation"):
        P._regrid_options({"interpolation": "sinc"})
    assert P._regrid_options(None) is None and P._regrid_options({}) == ("linear", 0.0)
    assert P._regrid_options({"interpolation": "bspline", "fill": -1}) == ("bspline", -1.0)
