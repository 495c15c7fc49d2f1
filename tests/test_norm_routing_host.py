"""CPU-only pins of the routing of the norm + act nodes (``Fn.NormActFn``, ``Fn.ResTailFn``): which ``ops`` launches a node
makes, in which order, with which operands -- where the statistics come from, which fused launch form runs, where the
gradients go, which dropout salt a node draws.  The ``ops`` wrappers are replaced by recorders that return CPU tensors of the
right shapes; everything else (the nodes, the hand-over tables, the gradient sinks, DropoutState) is the real code."""
import inspect

import pytest
import torch

from unet_bssfp_amd import functional as Fn
from unet_bssfp_amd import ops
from unet_bssfp_amd.gradsink import GradBuckets

BF16, F32 = torch.bfloat16, torch.float32
RECORDED = ("channel_stats", "norm_finalize", "normact_fwd", "normact_bwd", "normact_small_fwd", "normact_small_bwd", "restail_fwd",
            "maxpool2_bwd", "colsum", "colsum_into", "conv_fwd", "conv_wgrad", "weight_pack")
_SIGS = {name: inspect.signature(getattr(ops, name)) for name in RECORDED}
_NOT_FORMS = {"momentum", "want_affine"}        # always handed over: pinned by value where they matter, not as a form
BPG = 3                                         # blocks per statistics group the channel_stats stand-in reports
CPU = torch.device("cpu")
C, NCH = 32, 24                                 # padded / real channels of the activations


def _brief(v):
    if isinstance(v, torch.Tensor):
        return tuple(v.shape), str(v.dtype)[6:]
    if isinstance(v, (tuple, list)):
        return tuple(_brief(e) for e in v)
    return v


class Launch:
    """One recorded call: ``name``, ``args`` (the wrapper's own parameters, defaults filled in), ``forms`` (the optional parameters
    that were set to something other than their default) and ``ret`` (what the stand-in returned)."""

    def __init__(self, name, args, ret):
        self.name, self.args, self.ret = name, args, ret
        self.forms = set()
        for k, p in _SIGS[name].parameters.items():
            if p.default is inspect.Parameter.empty or k in _NOT_FORMS:
                continue
            v = args[k]
            if (v is not None) if p.default is None else (_brief(v) != _brief(p.default)):
                self.forms.add(k)

    def check(self, name, forms=(), **fields):
        assert self.name == name, (self.name, name)
        assert self.forms == set(forms), (name, sorted(self.forms))
        for k, want in fields.items():
            assert _brief(self.args[k]) == want, (name, k, _brief(self.args[k]), want)
        return self


def _same(a, b):
    """the same storage and shape (autograd may hand a node another Python object for one tensor)"""
    return a is not None and b is not None and a.data_ptr() == b.data_ptr() and a.shape == b.shape


def _returns(name, a):
    z = a.get("z")
    if name == "channel_stats":
        return torch.zeros((a["groups"] * BPG, 2, a["x"].shape[4])), BPG
    if name == "norm_finalize":
        return torch.zeros((a["groups"], a["c"])), torch.ones((a["groups"], a["c"]))
    if name == "normact_fwd":
        out = a["out"] if a["out"] is not None else torch.empty(z.shape, dtype=z.dtype)
        if a["pool"]:
            n, d, h, w, c = z.shape
            return out, torch.empty((n, d // 2, h // 2, w // 2, c), dtype=z.dtype), torch.empty((n, d // 2, h // 2, w // 2, c), dtype=torch.uint8)
        return out
    if name == "normact_small_fwd":
        out = a["out"] if a["out"] is not None else torch.empty(z.shape, dtype=z.dtype)
        return out, torch.zeros((a["groups"], z.shape[4])), torch.ones((a["groups"], z.shape[4]))
    if name in ("normact_bwd", "normact_small_bwd"):
        if name == "normact_bwd":
            fresh = (a["mean"] is not None and (a["batch_stats"] or a["want_affine_grads"] or a["dalpha"] is not None)
                     and a["affine_into"] is None)
        else:
            fresh = a["affine_into"] is None and a["want_affine"]
        dg, db = (torch.zeros(z.shape[4]), torch.zeros(z.shape[4])) if fresh else (None, None)
        return torch.empty(z.shape, dtype=z.dtype), dg, db
    if name == "restail_fwd":
        return torch.empty(z.shape, dtype=z.dtype)
    if name == "maxpool2_bwd":
        return torch.empty(a["x"].shape, dtype=a["x"].dtype)
    if name == "colsum":
        return torch.zeros(a["x"].shape[4])
    if name == "weight_pack":
        ops.LAST_WPACK_DESC[0] = None
        return torch.empty((1,)), a["coutp"] or 32, a["cinp"] or 16
    return None


@pytest.fixture
def rec(monkeypatch):
    """the launches made while the test runs, in order.  The hand-over tables are empty and the dropout salt is 0 before the
    test; DropoutState and torch's CPU generator are afterwards what they were."""
    launches = []

    def recorder(name):
        def call(*args, **kwargs):
            b = _SIGS[name].bind(*args, **kwargs)
            b.apply_defaults()
            a = dict(b.arguments)
            launches.append(Launch(name, a, _returns(name, a)))
            return launches[-1].ret
        return call

    for name in RECORDED:
        monkeypatch.setattr(ops, name, recorder(name))
    monkeypatch.setattr(Fn.Fp8Scales, "advance", classmethod(lambda cls, device: None))     # (device tables: no GPU here)
    saved = dict(Fn.DropoutState._base), Fn.DropoutState._salt
    Fn.DropoutState._base.pop(CPU, None)
    Fn.DropoutState._salt = 0
    for table in Fn.HandOver.per_step:
        table.clear()
    with torch.random.fork_rng(devices=[]):
        yield launches
    for table in Fn.HandOver.per_step:
        table.clear()
    Fn.DropoutState._base.clear()
    Fn.DropoutState._base.update(saved[0])
    Fn.DropoutState._salt = saved[1]


def _z(shape=(2, 4, 4, 4, C), dtype=F32):
    return torch.randn(shape, dtype=F32).to(dtype).requires_grad_()


def _affine(nch=NCH):
    return torch.nn.Parameter(torch.ones(nch)), torch.nn.Parameter(torch.zeros(nch))


def _running(nch=NCH):
    return torch.arange(nch, dtype=F32) / 8, torch.arange(nch, dtype=F32) / 4 + 0.5, torch.tensor(0, dtype=torch.long)


def _cfg(kind="instance", slope=0.1, p=0.0, act="leakyrelu", channels=NCH):
    return Fn.NormCfg(kind, channels, slope=slope, p=p, act=act)


def _slot(primed=True):
    s = Fn.Fp8Scales.Slot(torch.zeros(2), torch.zeros(1, dtype=torch.int32))
    s.primed = primed
    return s


# ---- the two call forms (the only part of this file that knows the nodes' argument order) ----------------------------------
def normact(z, cfg, training=True, part=None, gamma=None, beta=None, conv_bias=None, alpha=None, rm=None, rv=None, nbt=None,
            s2d_out=False, small=False, bn_groups=1, emit8=None, emit8_bwd=None, final=None, pool_after=False):
    return Fn.NormActFn.apply(z, part, gamma, beta, conv_bias, alpha, rm, rv, nbt, cfg, training,
                              Fn.NormOpts(s2d_out=s2d_out, small=small, bn_groups=bn_groups, emit8=emit8, emit8_bwd=emit8_bwd,
                                          final=final, pool_after=pool_after))


def restail(z, x, cfg, training=True, part=None, gamma=None, beta=None, conv_bias=None, rw=None, rb=None, spec=None, rm=None,
            rv=None, nbt=None):
    return Fn.ResTailFn.apply(z, part, x, gamma, beta, conv_bias, rw, rb, rm, rv, nbt, spec, cfg, training)


def _names(launches):
    return [l.name for l in launches]


# =========================================================================================== where the statistics come from
def test_instance_norm_without_partials_reduces_then_finalizes(rec):
    z, (g, b) = _z(), _affine()
    a = normact(z, _cfg(), gamma=g, beta=b)
    assert _names(rec) == ["channel_stats", "norm_finalize", "normact_fwd"]
    st = rec[0].check("channel_stats", groups=2)
    assert _same(st.args["x"], z)
    fin = rec[1].check("norm_finalize", parts_per_group=BPG, groups=2, c=C, count=64, shift=None, eps=1e-5, momentum=0.1, n_real=0)
    assert fin.args["part"] is st.ret[0]
    fwd = rec[2].check("normact_fwd", groups=2, mean=((2, C), "float32"), rstd=((2, C), "float32"), gamma=((NCH,), "float32"),
                       beta=((NCH,), "float32"), slope=0.1, drop_p=0.0, seed=0)
    assert fwd.args["mean"] is fin.ret[0] and fwd.args["rstd"] is fin.ret[1]
    assert _same(fwd.args["gamma"], g) and _same(fwd.args["beta"], b) and not fwd.args["gamma"].requires_grad
    del rec[:]
    a.backward(torch.ones_like(a))
    assert _names(rec) == ["normact_bwd"]
    bwd = rec[0].check("normact_bwd", groups=2, mean=((2, C), "float32"), rstd=((2, C), "float32"), slope=0.1, drop_p=0.0, seed=0,
                       batch_stats=True, want_affine_grads=True)
    assert bwd.args["mean"] is fin.ret[0] and _same(bwd.args["z"], z)
    assert z.grad is not None and g.grad.shape == (NCH,) and b.grad.shape == (NCH,)


def test_fused_partials_and_the_convolution_bias_as_shift(rec):
    z, (g, b) = _z(), _affine()
    part, bias = torch.zeros((8, 2, C)), torch.nn.Parameter(torch.zeros(NCH))
    normact(z, _cfg(), part=part, gamma=g, beta=b, conv_bias=bias)
    assert _names(rec) == ["norm_finalize", "normact_fwd"]
    fin = rec[0].check("norm_finalize", forms={"n_real"}, parts_per_group=4, groups=2, c=C, count=64, shift=((NCH,), "float32"),
                       n_real=NCH)
    assert _same(fin.args["part"], part) and _same(fin.args["shift"], bias) and not fin.args["shift"].requires_grad
    # an empty statistics tensor (what a convolution without fused statistics returns) counts as none
    del rec[:]
    normact(z, _cfg(), part=torch.empty((0,)), gamma=g, beta=b, conv_bias=bias)
    assert _names(rec) == ["channel_stats", "norm_finalize", "normact_fwd"]
    rec[1].check("norm_finalize", shift=None, n_real=0)


def test_batchnorm_training_updates_the_running_buffers_per_group(rec):
    z, (g, b), (rm, rv, nbt) = _z(), _affine(), _running()
    a = normact(z, _cfg("batch", 0.2), gamma=g, beta=b, rm=rm, rv=rv, nbt=nbt, bn_groups=2)
    assert _names(rec) == ["channel_stats", "norm_finalize", "normact_fwd"]
    rec[0].check("channel_stats", groups=2)
    fin = rec[1].check("norm_finalize", forms={"running_mean", "running_var", "n_real", "batches_tracked"}, groups=2, count=64,
                       shift=None, momentum=0.1, n_real=NCH)
    assert fin.args["running_mean"] is rm and fin.args["running_var"] is rv and fin.args["batches_tracked"] is nbt
    rec[2].check("normact_fwd", groups=2, mean=((2, C), "float32"), slope=0.2)
    del rec[:]
    a.backward(torch.ones_like(a))
    rec[0].check("normact_bwd", groups=2, batch_stats=True, want_affine_grads=True)


def test_batchnorm_training_without_running_buffers(rec):
    z, (g, b) = _z(), _affine()
    for training in (True, False):              # without running statistics eval mode normalises with the batch's as well
        del rec[:]
        a = normact(z, _cfg("batch"), training=training, gamma=g, beta=b)
        assert _names(rec) == ["channel_stats", "norm_finalize", "normact_fwd"]
        rec[0].check("channel_stats", groups=1)
        rec[1].check("norm_finalize", groups=1, count=128, shift=None, n_real=0)
        rec[2].check("normact_fwd", groups=1, mean=((1, C), "float32"))
        del rec[:]
        a.backward(torch.ones_like(a))
        rec[0].check("normact_bwd", groups=1, batch_stats=True, want_affine_grads=True)


def test_batchnorm_eval_takes_one_row_of_running_statistics_whatever_bn_groups(rec):
    z, (g, b), (rm, rv, nbt) = _z(), _affine(), _running()
    a = normact(z, _cfg("batch"), training=False, gamma=g, beta=b, rm=rm, rv=rv, nbt=None, bn_groups=2)
    assert _names(rec) == ["normact_fwd"]
    fwd = rec[0].check("normact_fwd", groups=1, mean=((1, C), "float32"), rstd=((1, C), "float32"))
    assert torch.equal(fwd.args["mean"][0, :NCH], rm) and not fwd.args["mean"][0, NCH:].any()
    want = torch.rsqrt(torch.cat([rv, torch.ones(C - NCH)]) + 1e-5)
    assert torch.equal(fwd.args["rstd"][0], want)
    assert rm[1] == 0.125 and nbt == 0
    del rec[:]
    a.backward(torch.ones_like(a))
    rec[0].check("normact_bwd", groups=1, mean=((1, C), "float32"), batch_stats=False, want_affine_grads=True)


def test_no_norm_launches_no_statistics_and_returns_no_affine_gradients(rec):
    z = _z()
    a = normact(z, _cfg("none", 0.2))
    assert _names(rec) == ["normact_fwd"]
    rec[0].check("normact_fwd", groups=1, mean=None, rstd=None, gamma=None, beta=None, slope=0.2)
    del rec[:]
    a.backward(torch.ones_like(a))
    assert _names(rec) == ["normact_bwd"]
    bwd = rec[0].check("normact_bwd", groups=1, mean=None, rstd=None, batch_stats=False, want_affine_grads=False)
    assert bwd.ret[1] is None and bwd.ret[2] is None


# =========================================================================================== which launch form runs
def test_small_is_one_launch_and_comes_first(rec):
    z, (g, b) = _z((2, 4, 4, 4, 64)), _affine(64)
    a = normact(z, _cfg(channels=64), gamma=g, beta=b, small=True)
    assert _names(rec) == ["normact_small_fwd"]
    rec[0].check("normact_small_fwd", groups=2, eps=1e-5, slope=0.1, momentum=0.1)
    del rec[:]
    a.backward(torch.ones_like(a))
    assert _names(rec) == ["normact_small_bwd"]
    bwd = rec[0].check("normact_small_bwd", groups=2, mean=((2, 64), "float32"), rstd=((2, 64), "float32"), slope=0.1, batch_stats=True,
                       want_affine=True)
    # every other form asked for at once: small still wins, nothing is handed over, the e4m3 slots stay untouched
    zb, (g, b), s8, s8b = _z((2, 4, 4, 4, C), BF16), _affine(), _slot(), _slot()
    fw = torch.nn.Parameter(torch.zeros(3, C, 1, 1, 1))
    del rec[:]
    a = normact(zb, _cfg(), gamma=g, beta=b, small=True, s2d_out=True, emit8=s8, emit8_bwd=s8b, final=(fw, None, False), pool_after=True)
    assert _names(rec) == ["normact_small_fwd"]
    fwd = rec[0].check("normact_small_fwd", forms={"out", "s2d"}, out=((2, 3, 3, 3, 8 * C), "bfloat16"))
    assert a.shape == (2, 3, 3, 3, 8 * C)
    assert not any(t._by_ptr for t in (Fn.Fp8Side, Fn.FusedFinal, Fn.PoolSide)) and not s8.touched
    del rec[:]
    a.backward(torch.ones_like(a))
    rec[0].check("normact_small_bwd", forms={"s2d"}, want_affine=True)
    assert not s8b.touched and not Fn.Fp8Side._by_ptr


def test_small_batchnorm_updates_the_running_buffers_in_its_launch(rec):
    z, (g, b), (rm, rv, nbt) = _z((2, 4, 4, 4, 64)), _affine(64), _running(64)
    normact(z, _cfg("batch", channels=64), gamma=g, beta=b, rm=rm, rv=rv, nbt=nbt, small=True, bn_groups=2)
    assert _names(rec) == ["normact_small_fwd"]
    fwd = rec[0].check("normact_small_fwd", forms={"running_mean", "running_var", "batches_tracked"}, groups=2, momentum=0.1)
    assert fwd.args["running_mean"] is rm and fwd.args["running_var"] is rv and fwd.args["batches_tracked"] is nbt


def test_small_without_batch_statistics_falls_back_to_the_streaming_launches(rec):
    z, (g, b), (rm, rv, _) = _z((2, 4, 4, 4, 64)), _affine(64), _running(64)
    a = normact(z, _cfg("none", channels=64), small=True)
    assert _names(rec) == ["normact_fwd"]
    rec[0].check("normact_fwd", mean=None)
    del rec[:]
    a.backward(torch.ones_like(a))
    assert _names(rec) == ["normact_bwd"]
    del rec[:]
    a = normact(z, _cfg("batch", channels=64), training=False, gamma=g, beta=b, rm=rm, rv=rv, small=True)
    assert _names(rec) == ["normact_fwd"]
    rec[0].check("normact_fwd", groups=1, mean=((1, 64), "float32"))
    del rec[:]
    a.backward(torch.ones_like(a))
    assert _names(rec) == ["normact_bwd"]


def test_a_node_asked_for_the_small_kernel_writes_no_e4m3_copy_even_where_it_falls_back(rec):
    z, (g, b), (rm, rv, _), s8, s8b = _z(dtype=BF16), _affine(), _running(), _slot(), _slot()
    fw = torch.nn.Parameter(torch.zeros(3, C, 1, 1, 1))
    a = normact(z, _cfg("batch"), training=False, gamma=g, beta=b, rm=rm, rv=rv, small=True, emit8=s8, emit8_bwd=s8b,
                final=(fw, None, False))
    assert _names(rec) == ["normact_fwd"]
    rec[0].check("normact_fwd", forms={"final"}, groups=1, mean=((1, C), "float32"))      # ... but the later forms are served
    assert not s8.touched and not Fn.Fp8Side._by_ptr
    del rec[:]
    a.backward(torch.ones_like(a))
    rec[0].check("normact_bwd", batch_stats=False)
    assert not s8b.touched and not Fn.Fp8Side._by_ptr


def test_s2d_comes_before_emit8_final_and_pool(rec):
    z, (g, b), s8, s8b = _z(dtype=BF16), _affine(), _slot(), _slot()
    fw = torch.nn.Parameter(torch.zeros(3, C, 1, 1, 1))
    a = normact(z, _cfg(), gamma=g, beta=b, s2d_out=True, emit8=s8, emit8_bwd=s8b, final=(fw, None, False), pool_after=True)
    assert _names(rec) == ["channel_stats", "norm_finalize", "normact_fwd"]
    fwd = rec[2].check("normact_fwd", forms={"out", "s2d"}, out=((2, 3, 3, 3, 8 * C), "bfloat16"), s2d=True)
    assert a is fwd.args["out"] or _same(a, fwd.args["out"])
    assert not any(t._by_ptr for t in (Fn.Fp8Side, Fn.FusedFinal, Fn.PoolSide)) and not s8.touched
    del rec[:]
    a.backward(torch.ones_like(a))
    rec[0].check("normact_bwd", forms={"s2d"}, s2d=True, batch_stats=True)
    assert not s8b.touched and not Fn.Fp8Side._by_ptr


def test_emit8_writes_the_e4m3_copy_and_hands_it_over(rec):
    z, (g, b), s8 = _z(dtype=BF16), _affine(), _slot()
    fw = torch.nn.Parameter(torch.zeros(3, C, 1, 1, 1))
    a = normact(z, _cfg(), gamma=g, beta=b, emit8=s8, final=(fw, None, False), pool_after=True)
    fwd = rec[2].check("normact_fwd", forms={"q8"}, q8=(((2, 4, 4, 4, C), "uint8"), ((1,), "float32"), ((1,), "float32")))
    a8, use, nxt = fwd.args["q8"]
    assert _same(use, s8.use) and _same(nxt, s8.next) and s8.touched
    assert not Fn.FusedFinal._by_ptr and not Fn.PoolSide._by_ptr
    hit = Fn.Fp8Side.take(a)
    assert len(hit) == 1 and hit[0] is a8 and not Fn.Fp8Side._by_ptr


@pytest.mark.parametrize("why", ["unprimed", "c64", "f32", "s2d_out"])
def test_emit8_that_cannot_be_served_gives_no_e4m3_copy(rec, why):
    dtype = F32 if why == "f32" else BF16
    c = 64 if why == "c64" else C
    z, (g, b), s8 = _z((2, 4, 4, 4, c), dtype), _affine(c), _slot(primed=why != "unprimed")
    a = normact(z, _cfg(channels=c), gamma=g, beta=b, emit8=s8, s2d_out=why == "s2d_out")
    rec[2].check("normact_fwd", forms={"out", "s2d"} if why == "s2d_out" else ())
    assert not s8.touched and Fn.Fp8Side.take(a) is None


def test_an_unserved_emit8_leaves_the_later_forms_their_turn(rec):
    z, (g, b), s8 = _z(dtype=BF16), _affine(), _slot(primed=False)
    fw = torch.nn.Parameter(torch.zeros(3, C, 1, 1, 1))
    normact(z, _cfg(), gamma=g, beta=b, emit8=s8, final=(fw, None, False), pool_after=True)
    rec[2].check("normact_fwd", forms={"final"})
    del rec[:]
    normact(z, _cfg(), gamma=g, beta=b, emit8=s8, pool_after=True)
    rec[2].check("normact_fwd", forms={"pool"})


@pytest.mark.parametrize("skip_a", [False, True])
def test_final_evaluates_the_1x1x1_convolution_and_hands_its_output_over(rec, skip_a):
    z, (g, b) = _z(dtype=BF16), _affine()
    fw, fb = torch.nn.Parameter(torch.zeros(3, C, 1, 1, 1)), torch.nn.Parameter(torch.zeros(3))
    a = normact(z, _cfg(), gamma=g, beta=b, final=(fw, fb, skip_a), pool_after=True)
    fwd = rec[2].check("normact_fwd", forms={"final", "skip_a"} if skip_a else {"final"}, skip_a=skip_a,
                       final=(((3, C, 1, 1, 1), "float32"), ((3,), "float32"), ((2, 4, 4, 4, 16), "bfloat16")))
    w_, b_, y = fwd.args["final"]
    assert _same(w_, fw) and _same(b_, fb) and not w_.requires_grad and not b_.requires_grad
    assert not Fn.PoolSide._by_ptr
    assert Fn.FusedFinal.take(a, fw) is y and not Fn.FusedFinal._by_ptr
    del rec[:]
    a = normact(z, _cfg(), gamma=g, beta=b, final=(fw, None, skip_a))         # a convolution without bias
    assert rec[2].args["final"][1] is None


@pytest.mark.parametrize("why", ["f32", "c64"])
def test_final_that_cannot_be_served_gives_the_plain_form(rec, why):
    c = 64 if why == "c64" else C
    z, (g, b) = _z((2, 4, 4, 4, c), F32 if why == "f32" else BF16), _affine(c)
    fw = torch.nn.Parameter(torch.zeros(3, c, 1, 1, 1))
    a = normact(z, _cfg(channels=c), gamma=g, beta=b, final=(fw, None, False))
    rec[2].check("normact_fwd")
    assert Fn.FusedFinal.take(a, fw) is None
    del rec[:]
    normact(z, _cfg(channels=c), gamma=g, beta=b, final=(fw, None, False), pool_after=True)
    rec[2].check("normact_fwd", forms={"pool"})


def test_pool_after_pools_in_the_launch_and_hands_the_result_over(rec):
    z, (g, b) = _z(), _affine()
    a = normact(z, _cfg(), gamma=g, beta=b, pool_after=True)
    fwd = rec[2].check("normact_fwd", forms={"pool"}, pool=True)
    hit = Fn.PoolSide.take(a)
    assert len(hit) == 2 and hit[0] is fwd.ret[1] and hit[1] is fwd.ret[2] and _same(a, fwd.ret[0])


@pytest.mark.parametrize("why", ["odd", "disabled"])
def test_pool_after_that_cannot_be_served_gives_the_plain_form(rec, why, monkeypatch):
    if why == "disabled":
        monkeypatch.setattr(Fn.PoolSide, "enabled", False)
    z, (g, b) = _z((2, 4, 4, 3, C) if why == "odd" else (2, 4, 4, 4, C)), _affine()
    a = normact(z, _cfg(), gamma=g, beta=b, pool_after=True)
    rec[2].check("normact_fwd")
    assert Fn.PoolSide.take(a) is None


@pytest.mark.parametrize("why", [None, "unprimed", "f32", "c64"])
def test_emit8_bwd_writes_the_e4m3_copy_of_dz_on_the_streaming_path(rec, why):
    c = 64 if why == "c64" else C
    z, (g, b), s8b = _z((2, 4, 4, 4, c), F32 if why == "f32" else BF16), _affine(c), _slot(primed=why != "unprimed")
    a = normact(z, _cfg(channels=c), gamma=g, beta=b, emit8_bwd=s8b)
    rec[2].check("normact_fwd")
    del rec[:]
    a.backward(torch.ones_like(a))
    if why is not None:
        rec[0].check("normact_bwd")
        assert not s8b.touched and not Fn.Fp8Side._by_ptr
        return
    bwd = rec[0].check("normact_bwd", forms={"q8"}, q8=(((2, 4, 4, 4, C), "uint8"), ((1,), "float32"), ((1,), "float32")))
    assert _same(bwd.args["q8"][1], s8b.use) and _same(bwd.args["q8"][2], s8b.next) and s8b.touched
    hit = Fn.Fp8Side.take(bwd.ret[0])
    assert hit[0] is bwd.args["q8"][0]


# =========================================================================================== backward: lazy gradients
def test_a_lazy_dx_placeholder_becomes_the_implicit_form(rec):
    z, (g, b) = _z(dtype=BF16), _affine()
    a = normact(z, _cfg(), gamma=g, beta=b)
    ph, gz, gw = torch.empty_like(a), torch.zeros((2, 4, 4, 4, 16), dtype=BF16), torch.zeros(3, C, 1, 1, 1)
    Fn.LazyDx.put(ph, gz, gw)
    del rec[:]
    a.backward(ph)
    assert _names(rec) == ["normact_bwd"]
    bwd = rec[0].check("normact_bwd", forms={"implicit"}, da=None, implicit=(_brief(gz), _brief(gw)))
    assert bwd.args["implicit"][0] is gz and bwd.args["implicit"][1] is gw and not Fn.LazyDx._by_ptr


@pytest.mark.parametrize("how", ["small", "s2d_out"])
def test_a_lazy_dx_placeholder_at_a_node_that_cannot_form_it_is_an_error(rec, how):
    z, (g, b) = _z((2, 4, 4, 4, 64), BF16), _affine(64)
    a = normact(z, _cfg(channels=64), gamma=g, beta=b, small=how == "small", s2d_out=how == "s2d_out")
    ph = torch.empty_like(a)
    Fn.LazyDx.put(ph, torch.zeros((2, 4, 4, 4, 16), dtype=BF16), torch.zeros(3, 64, 1, 1, 1))
    del rec[:]
    with pytest.raises(RuntimeError, match="LazyDx placeholder reached a norm node that cannot form the gradient itself"):
        a.backward(ph)
    assert not rec


def _lazy_pool(a, x_shape, dtype):
    n, d, h, w, c = x_shape
    ph = torch.empty_like(a)
    x, y = torch.zeros(x_shape, dtype=dtype), torch.zeros((n, d // 2, h // 2, w // 2, c), dtype=dtype)
    idx, d_pool, d_skip = torch.zeros(y.shape, dtype=torch.uint8), torch.zeros_like(y), torch.zeros_like(x)
    Fn.LazyPool.put(ph, x, y, idx, d_pool, d_skip)
    return ph, (x, y, idx, d_pool, d_skip)


def test_a_lazy_pool_placeholder_becomes_the_pool_form_on_the_streaming_path(rec):
    z, (g, b) = _z(), _affine()
    a = normact(z, _cfg(), gamma=g, beta=b)
    ph, (x, y, idx, d_pool, d_skip) = _lazy_pool(a, z.shape, F32)
    del rec[:]
    a.backward(ph)
    assert _names(rec) == ["normact_bwd"]
    bwd = rec[0].check("normact_bwd", forms={"pool"})
    assert bwd.args["pool"][0] is idx and bwd.args["pool"][1] is d_pool and bwd.args["da"] is d_skip and not Fn.LazyPool._by_ptr


@pytest.mark.parametrize("how", ["small", "s2d_out"])
def test_a_lazy_pool_placeholder_is_materialised_for_the_small_and_s2d_kernels(rec, how):
    z, (g, b) = _z((2, 4, 4, 4, 64)), _affine(64)
    a = normact(z, _cfg(channels=64), gamma=g, beta=b, small=how == "small", s2d_out=how == "s2d_out")
    ph, (x, y, idx, d_pool, d_skip) = _lazy_pool(a, z.shape, F32)
    del rec[:]
    a.backward(ph)
    assert _names(rec) == ["maxpool2_bwd", "normact_small_bwd" if how == "small" else "normact_bwd"]
    mp = rec[0].check("maxpool2_bwd", forms={"add"})
    assert mp.args["x"] is x and mp.args["y"] is y and mp.args["dy"] is d_pool and mp.args["add"] is d_skip
    rec[1].check(rec[1].name, forms={"s2d"} if how == "s2d_out" else ())
    assert rec[1].args["da"] is mp.ret


# =========================================================================================== backward: where the gradients go
@pytest.mark.parametrize("small", [False, True])
def test_affine_gradients_fresh_then_into_the_sink_then_accumulated(rec, small):
    c = 64 if small else C
    nch = 64 if small else NCH
    name = "normact_small_bwd" if small else "normact_bwd"

    def run(g, b):
        z = _z((2, 4, 4, 4, c))
        a = normact(z, _cfg(channels=nch), gamma=g, beta=b, small=small)
        del rec[:]
        a.backward(torch.ones_like(a))
        assert _names(rec) == [name]
        return rec[0]

    g, b = _affine(nch)
    bwd = run(g, b).check(name)                          # no sink: fresh tensors go back to autograd, cut to the real channels
    assert bwd.ret[1].shape == (c,) and g.grad.shape == (nch,) and b.grad.shape == (nch,)
    g, b = _affine(nch)
    sink = GradBuckets([[g, b]], uses_per_phase=2)
    sink.begin_phase()
    first = run(g, b).check(name, forms={"affine_into"}, accumulate=False)
    assert first.args["affine_into"][0].data_ptr() == g.grad.data_ptr() and first.args["affine_into"][1].data_ptr() == b.grad.data_ptr()
    assert not sink.fresh(g) and not sink.fresh(b) and not sink.complete()
    second = run(g, b).check(name, forms={"affine_into", "accumulate"}, accumulate=True)
    assert second.args["affine_into"][0].data_ptr() == g.grad.data_ptr() and second.args["affine_into"][1].data_ptr() == b.grad.data_ptr()
    assert sink.complete()
    # gamma and beta in different sinks: no sink at all
    g, b = _affine(nch)
    sg, sb = GradBuckets([[g]]), GradBuckets([[b]])
    sg.begin_phase(), sb.begin_phase()
    run(g, b).check(name)
    assert sg.fresh(g) and sb.fresh(b)


def test_only_one_affine_gradient_wanted_bypasses_the_sink(rec):
    z, (g, b) = _z(), _affine()
    sink = GradBuckets([[g, b]])
    sink.begin_phase()
    b.requires_grad_(False)
    a = normact(z, _cfg(), gamma=g, beta=b)
    del rec[:]
    a.backward(torch.ones_like(a))
    rec[0].check("normact_bwd", want_affine_grads=True)
    assert sink.fresh(g)


@pytest.mark.parametrize("small", [False, True])
def test_prelu_slope_gradient_goes_straight_to_its_target_or_through_a_scalar(rec, small):
    c = 64 if small else C
    nch = 64 if small else NCH
    name = "normact_small_bwd" if small else "normact_bwd"
    (g, b), alpha = _affine(nch), torch.nn.Parameter(torch.full((1,), 0.25))
    sink, asink = GradBuckets([[g, b]], uses_per_phase=2), GradBuckets([[alpha]])
    sink.begin_phase(), asink.begin_phase()

    def run():
        z = _z((2, 4, 4, 4, c))
        a = normact(z, _cfg(act="prelu", channels=nch), gamma=g, beta=b, alpha=alpha, small=small)
        fwd = rec[-1]
        assert _same(fwd.args["alpha"], alpha) and not fwd.args["alpha"].requires_grad and "alpha" in fwd.forms
        del rec[:]
        a.backward(torch.ones_like(a))
        assert _names(rec) == [name]
        return rec[0]

    first = run().check(name, forms={"affine_into", "alpha", "dalpha"}, accumulate=False, dalpha=((1,), "float32"))
    assert first.args["dalpha"].data_ptr() == alpha.grad.data_ptr() and not asink.fresh(alpha)
    asink.begin_phase()                                  # the slope starts afresh, the affine pair is at its second use
    alpha.grad.fill_(7.0)
    second = run().check(name, forms={"affine_into", "accumulate", "alpha", "dalpha"}, accumulate=True, dalpha=((1,), "float32"))
    assert second.args["dalpha"].data_ptr() != alpha.grad.data_ptr() and not second.args["dalpha"].any()
    assert alpha.grad.item() == 0.0 and not asink.fresh(alpha)         # the (zero) scalar was copied over the stale value
    # ... and the other way round: the slope accumulates, the affine pair is written
    sink.begin_phase()
    asink.begin_phase(2)
    asink.written(alpha)
    alpha.grad.fill_(7.0)
    third = run().check(name, forms={"affine_into", "alpha", "dalpha"}, accumulate=False)
    assert third.args["dalpha"].data_ptr() != alpha.grad.data_ptr() and alpha.grad.item() == 7.0


def test_prelu_slope_gradient_without_sinks_is_a_fresh_tensor(rec):
    z, (g, b), alpha = _z(), _affine(), torch.nn.Parameter(torch.full((1,), 0.25))
    a = normact(z, _cfg(act="prelu"), gamma=g, beta=b, alpha=alpha)
    del rec[:]
    a.backward(torch.ones_like(a))
    rec[0].check("normact_bwd", forms={"alpha", "dalpha"}, dalpha=((1,), "float32"))
    assert alpha.grad.shape == (1,)
    # a frozen slope: read by the kernels, no gradient asked for
    alpha.requires_grad_(False)
    a = normact(z, _cfg(act="prelu"), gamma=g, beta=b, alpha=alpha)
    del rec[:]
    a.backward(torch.ones_like(a))
    rec[0].check("normact_bwd", forms={"alpha"})


# =========================================================================================== dropout salts
def test_dropout_salts_count_the_nodes_that_drop_within_a_step(rec):
    (g, b) = _affine()
    base = Fn.DropoutState.base(CPU)

    def seed_of(p, training=True, small=False):
        del rec[:]
        c = 64 if small else C
        a = normact(_z((2, 4, 4, 4, c)), _cfg(p=p, channels=c), training=training, gamma=_affine(c)[0], beta=_affine(c)[1], small=small)
        fwd = rec[-1]
        del rec[:]
        a.backward(torch.ones_like(a))
        bwd = rec[0]
        assert bwd.args["seed"] == fwd.args["seed"] and bwd.args["drop_p"] == fwd.args["drop_p"]
        assert bwd.args["seed_t"] is fwd.args["seed_t"]
        assert (fwd.args["seed_t"] is base) if fwd.args["seed"] else (fwd.args["seed_t"] is None)
        return fwd.args["drop_p"], fwd.args["seed"]

    assert seed_of(0.1) == (0.1, 1)
    assert seed_of(0.0) == (0.0, 0)                      # a node that drops nothing consumes no salt
    assert seed_of(0.1, training=False) == (0.0, 0)      # nor does one in eval mode
    assert seed_of(0.25, small=True) == (0.25, 2)
    assert seed_of(0.1) == (0.1, 3)
    before = int(base)
    Fn.begin_step(CPU)
    assert Fn.DropoutState.base(CPU) is base and int(base) == before + 1
    assert seed_of(0.1) == (0.1, 1)                      # a new step starts at 1 again


# =========================================================================================== errors
def test_prelu_and_alpha_come_together_and_with_a_norm(rec):
    z, (g, b), alpha = _z(), _affine(), torch.nn.Parameter(torch.full((1,), 0.25))
    with pytest.raises(ValueError, match="a PReLU node takes its slope as `alpha`"):
        normact(z, _cfg(act="prelu"), gamma=g, beta=b)
    with pytest.raises(ValueError, match="a PReLU node takes its slope as `alpha`"):
        normact(z, _cfg(), gamma=g, beta=b, alpha=alpha)
    with pytest.raises(ValueError, match="a PReLU node takes its slope as `alpha`"):
        normact(z, _cfg("none", act="prelu"), alpha=alpha)
    assert not rec


def test_one_value_per_channel_in_training_is_an_error(rec):
    g, b = _affine()
    rm, rv, nbt = _running()
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        normact(_z((2, 1, 1, 1, C)), _cfg(), gamma=g, beta=b)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        normact(_z((1, 1, 1, 1, C)), _cfg("batch"), gamma=g, beta=b, rm=rm, rv=rv, nbt=nbt)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        normact(_z((2, 1, 1, 1, C)), _cfg("batch"), gamma=g, beta=b, rm=rm, rv=rv, nbt=nbt, bn_groups=2)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        normact(_z((2, 1, 1, 1, 64)), _cfg(channels=64), gamma=_affine(64)[0], beta=_affine(64)[1], small=True)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        restail(_z((1, 1, 1, 1, C)), _z((1, 1, 1, 1, C)), _cfg("batch", 0.0), gamma=g, beta=b, rm=rm, rv=rv, nbt=nbt)
    assert not rec
    normact(_z((1, 1, 1, 1, C)), _cfg("batch"), training=False, gamma=g, beta=b, rm=rm, rv=rv)       # eval: running statistics
    normact(_z((1, 1, 1, 1, C)), _cfg("none"))
    assert _names(rec) == ["normact_fwd", "normact_fwd"]


def test_restail_takes_a_norm_with_relu_and_no_dropout(rec):
    g, b = _affine()
    for cfg in (_cfg("none", 0.0), _cfg("batch", 0.1), _cfg("batch", 0.0, p=0.1), _cfg("batch", 0.0, act="prelu")):
        with pytest.raises(ValueError, match="a norm followed by ReLU, without dropout"):
            restail(_z(), _z(), cfg, gamma=g, beta=b)
    assert not rec


# =========================================================================================== the residual tail
@pytest.mark.parametrize("sinks", [False, True])
@pytest.mark.parametrize("training", [True, False])
def test_restail_with_the_identity_residual(rec, training, sinks):
    z, x, (g, b), (rm, rv, nbt) = _z(), _z(), _affine(), _running()
    part, bias = torch.zeros((8, 2, C)), torch.nn.Parameter(torch.zeros(NCH))
    if sinks:
        sink = GradBuckets([[g, b]], uses_per_phase=2)
        sink.begin_phase()
    y = restail(z, x, _cfg("batch", 0.0), training=training, part=part, gamma=g, beta=b, conv_bias=bias, rm=rm, rv=rv,
                nbt=nbt if training else None)
    if training:
        assert _names(rec) == ["norm_finalize", "restail_fwd"]
        fin = rec[0].check("norm_finalize", forms={"running_mean", "running_var", "n_real", "batches_tracked"}, parts_per_group=8,
                           groups=1, c=C, count=128, shift=((NCH,), "float32"), eps=1e-5, momentum=0.1, n_real=NCH)
        assert _same(fin.args["part"], part) and _same(fin.args["shift"], bias)
        assert fin.args["running_mean"] is rm and fin.args["running_var"] is rv and fin.args["batches_tracked"] is nbt
    else:
        assert _names(rec) == ["restail_fwd"]
    fwd = rec[-1].check("restail_fwd", groups=1, mean=((1, C), "float32"), rstd=((1, C), "float32"), gamma=((NCH,), "float32"),
                        beta=((NCH,), "float32"), n_real=NCH, cx=NCH)
    assert _same(fwd.args["z"], z) and _same(fwd.args["x"], x) and _same(fwd.args["gamma"], g) and _same(fwd.args["beta"], b)
    if training:
        assert fwd.args["mean"] is fin.ret[0] and fwd.args["rstd"] is fin.ret[1]
    else:
        assert torch.equal(fwd.args["mean"][0, :NCH], rm) and not fwd.args["mean"][0, NCH:].any()
        assert torch.equal(fwd.args["rstd"][0], torch.rsqrt(torch.cat([rv, torch.ones(C - NCH)]) + 1e-5))
    for use in range(2 if sinks else 1):
        del rec[:]
        dy = torch.ones_like(y)
        y.backward(dy, retain_graph=True)
        assert _names(rec) == ["normact_bwd"]
        forms = ({"affine_into", "accumulate"} if use else {"affine_into"}) if sinks else ()
        bwd = rec[0].check("normact_bwd", forms=forms, groups=1, mean=((1, C), "float32"), slope=0.0, drop_p=0.0, seed=0,
                           batch_stats=training, want_affine_grads=True, accumulate=bool(use))
        assert _same(bwd.args["z"], z) and _same(bwd.args["da"], dy) and bwd.args["mean"] is fwd.args["mean"]
        if sinks:
            assert bwd.args["affine_into"][0].data_ptr() == g.grad.data_ptr() and bwd.args["affine_into"][1].data_ptr() == b.grad.data_ptr()
    assert torch.equal(x.grad, torch.full_like(x, 2.0 if sinks else 1.0))      # the identity branch: dx is dy itself
    assert not sinks or sink.complete()


def test_restail_reduces_the_statistics_itself_without_partials(rec):
    z, x, (g, b) = _z(), _z(), _affine()
    y = restail(z, x, _cfg("instance", 0.0), training=False, gamma=g, beta=b)         # instance norm: the batch's statistics in eval too
    assert _names(rec) == ["channel_stats", "norm_finalize", "restail_fwd"]
    rec[0].check("channel_stats", groups=2)
    rec[1].check("norm_finalize", parts_per_group=BPG, groups=2, c=C, count=64, shift=None, n_real=0)
    rec[2].check("restail_fwd", groups=2, mean=((2, C), "float32"))
    del rec[:]
    y.backward(torch.ones_like(y))
    rec[0].check("normact_bwd", groups=2, batch_stats=True, want_affine_grads=True)
    # BatchNorm without running statistics: batch statistics, nothing to update
    del rec[:]
    restail(z, x, _cfg("batch", 0.0), training=False, gamma=g, beta=b)
    assert _names(rec) == ["channel_stats", "norm_finalize", "restail_fwd"]
    rec[1].check("norm_finalize", groups=1, count=128)


@pytest.mark.parametrize("sinks", [False, True])
@pytest.mark.parametrize("training", [True, False])
def test_restail_with_the_projection_residual(rec, training, sinks):
    cin = 5
    z, x, (g, b), (rm, rv, nbt) = _z(), _z((2, 4, 4, 4, 16)), _affine(), _running()
    spec = Fn.ConvSpec("conv", cin, NCH, 1, 1, 0)
    rw, rb = torch.nn.Parameter(torch.zeros(NCH, cin, 1, 1, 1)), torch.nn.Parameter(torch.zeros(NCH))
    if sinks:
        sink = GradBuckets([[g, b, rw, rb]], uses_per_phase=2)
        sink.begin_phase()
    y = restail(z, x, _cfg("batch", 0.0), training=training, gamma=g, beta=b, rw=rw, rb=rb, spec=spec, rm=rm, rv=rv,
                nbt=nbt if training else None)
    assert _names(rec) == (["channel_stats", "norm_finalize", "restail_fwd"] if training else ["restail_fwd"])
    if training:
        rec[1].check("norm_finalize", forms={"running_mean", "running_var", "n_real", "batches_tracked"}, parts_per_group=BPG, groups=1,
                     count=128, shift=None, n_real=NCH)
    fwd = rec[-1].check("restail_fwd", forms={"rw", "rb"}, groups=1, n_real=NCH, cx=cin, rw=((NCH, cin, 1, 1, 1), "float32"),
                        rb=((NCH,), "float32"))
    assert _same(fwd.args["rw"], rw) and _same(fwd.args["rb"], rb) and not fwd.args["rw"].requires_grad
    for use in range(2 if sinks else 1):
        del rec[:]
        dy = torch.ones_like(y)
        y.backward(dy, retain_graph=True)
        assert _names(rec) == ["normact_bwd"] + (["weight_pack"] if use == 0 else []) + ["conv_fwd", "conv_wgrad",
                                                                                         "colsum_into" if sinks else "colsum"]
        acc = bool(use)
        rec[0].check("normact_bwd", forms=({"affine_into", "accumulate"} if use else {"affine_into"}) if sinks else (), slope=0.0,
                     drop_p=0.0, seed=0, batch_stats=training, want_affine_grads=True)
        if use == 0:                                     # the 1x1x1 data gradient's packing: (cin, cout) swapped, taps reversed
            pack = rec[1].check("weight_pack", forms={"cinp"}, cout=cin, cin=NCH, ks=1, s_co=1, s_ci=cin, s_k=(1, 1, 1), tbase=(0, 0, 0),
                         tstep=(-1, -1, -1), dtype=F32, cinp=C)
        dgrad = rec[-3].check("conv_fwd", forms={"real"}, x1=None, bias=None, ks=1, stride=1, pad=(0, 0, 0),
                              out=((2, 4, 4, 4, 16), "float32"), grid=(4, 4, 4), real=(NCH, cin))
        assert _same(dgrad.args["x0"], dy) and dgrad.args["wp"] is pack.ret[0] and dgrad.args["coutp"] == pack.ret[1]
        wg = rec[-2].check("conv_wgrad", forms={"accumulate"} if acc else (), x1=None, grid=(4, 4, 4), gs=1, goff=(0, 0, 0), ks=1, stride=1,
                           pad=(0, 0, 0), cout=NCH, cin=cin, s_co=cin, s_ci=1, s_k=(1, 1, 1), tbase=(0, 0, 0), tstep=(1, 1, 1),
                           accumulate=acc, defer=None)
        assert _same(wg.args["x0"], x) and _same(wg.args["g"], dy)
        if sinks:
            assert wg.args["dw"].data_ptr() == rw.grad.data_ptr()
            cs = rec[-1].check("colsum_into", accumulate=acc)
            assert _same(cs.args["x"], dy) and cs.args["out"].data_ptr() == rb.grad.data_ptr()
        else:
            assert _same(rec[-1].check("colsum").args["x"], dy)
            assert rw.grad.shape == rw.shape and rb.grad.shape == (NCH,)
    assert x.grad.shape == x.shape
    assert not sinks or sink.complete()


def test_restail_backward_launches_only_what_is_needed(rec):
    z, x, (g, b) = _z(), torch.randn((2, 4, 4, 4, 16)), _affine()
    spec = Fn.ConvSpec("conv", 5, NCH, 1, 1, 0)
    rw, rb = torch.nn.Parameter(torch.zeros(NCH, 5, 1, 1, 1)), torch.nn.Parameter(torch.zeros(NCH))
    rw.requires_grad_(False)
    y = restail(z, x, _cfg("instance", 0.0), gamma=g, beta=b, rw=rw, rb=rb, spec=spec)
    del rec[:]
    y.backward(torch.ones_like(y))
    assert _names(rec) == ["normact_bwd", "colsum"]


# =========================================================================================== the positional form of older callers
def _records(launches):
    return [(l.name, sorted(l.forms), {k: _brief(v) for k, v in l.args.items()}) for l in launches]


def test_the_older_positional_calls_are_served_like_the_named_ones(rec):
    (g, b), (rm, rv, nbt), alpha = _affine(64), _running(64), torch.nn.Parameter(torch.full((1,), 0.25))
    fw, s8 = torch.nn.Parameter(torch.zeros(3, C, 1, 1, 1)), _slot()
    g24, b24 = _affine()
    z64, zb = _z((2, 4, 4, 4, 64)), _z(dtype=BF16)
    pairs = [
        (lambda: normact(z64, _cfg("batch", channels=64), gamma=g, beta=b, rm=rm, rv=rv, nbt=nbt, small=True, bn_groups=2, s2d_out=True),
         lambda: Fn.NormActFn.apply(z64, None, g, b, None, _cfg("batch", channels=64), True, rm, rv, True, nbt, True, 2)),
        (lambda: normact(zb, _cfg(act="prelu"), gamma=g24, beta=b24, alpha=alpha, emit8_bwd=s8, final=(fw, None, False), pool_after=True),
         lambda: Fn.NormActFn.apply(zb, None, g24, b24, None, _cfg(act="prelu"), True, None, None, False, None, False, 1, None, s8,
                                    (fw, None, False), True, alpha)),
        (lambda: normact(zb, _cfg("none")), lambda: Fn.NormActFn.apply(zb, None, None, None, None, _cfg("none"), True, None, None)),
        (lambda: restail(zb, zb, _cfg("batch", 0.0), gamma=g24, beta=b24, rm=rm[:NCH], rv=rv[:NCH], nbt=nbt),
         lambda: Fn.ResTailFn.apply(zb, None, zb, g24, b24, None, None, None, None, _cfg("batch", 0.0), True, rm[:NCH], rv[:NCH], nbt)),
        (lambda: restail(zb, zb, _cfg("instance", 0.0), gamma=g24, beta=b24),
         lambda: Fn.ResTailFn.apply(zb, None, zb, g24, b24, None, None, None, None, _cfg("instance", 0.0), True, None, None)),
    ]
    for named, positional in pairs:
        got = []
        for call in (named, positional):
            del rec[:]
            Fn.DropoutState._salt = 0
            y = call()
            y.backward(torch.ones_like(y))
            got.append(_records(rec))
            for table in Fn.HandOver.per_step:
                table.clear()
        assert len(got[0]) >= 2 and len(got[0]) == len(got[1])
        for a, p in zip(*got):
            assert a[0] == p[0] and a[1] == p[1] and a[2] == p[2], (a[0], a[1], p[1])
