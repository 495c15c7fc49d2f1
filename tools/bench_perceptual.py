"""losses.PerceptualLoss forward at the reference's real shape -- prediction and target of 8 x 6 x 64^3, 48 network samples per
tensor, 96 in all -- whole and by part, the achieved FLOP/s of its convolutions against the bf16 MFMA peak, and the same extractor run by
stock torch in bf16 (channels-last Conv3d + eval BatchNorm3d modules) on the same GPU.  Device events, warm-up, interleaved
rounds in one process; one JSON line per measurement (median and min over the rounds, ms).

    python tools/bench_perceptual.py [--parts ours,stock] [--reps 10] [--batch 8] [--channels 6] [--size 64] [--lib LIB]

``--parts backward,stock_backward`` measures the backward with respect to the prediction the same way: whole and by part (tail,
every block's data-gradient launches, pool, stem, normalisation), a data gradient counted with its forward's FLOPs, next to the
same network's backward with respect to its input in stock torch (bf16, channels-last, autograd).
"""
import argparse
import copy
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unet_bssfp_amd import ops                                           # noqa: E402
from unet_bssfp_amd.losses import PerceptualLoss                         # noqa: E402
from unet_bssfp_amd.medicalnet import BLOCKS, MedicalNetResNet10, medicalnet_backward   # noqa: E402

PEAK_BF16_FLOPS = 2.5e15                                                 # MI355X dense bf16 MFMA (spec)


def rounds(fns, reps, warmup=3):
    """{name: [ms per call] * reps}: every variant once per round, in turn"""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            out[k].append(e0.elapsed_time(e1))
    return out


def report(what, times, flops=None):
    med = {}
    for k, v in times.items():
        med[k] = statistics.median(v)
        row = dict(what=what, variant=k, median_ms=round(med[k], 4), min_ms=round(min(v), 4), reps=len(v))
        if flops and flops.get(k):
            row["gflop"] = round(flops[k] / 1e9, 2)
            row["tflops"] = round(flops[k] / med[k] / 1e9, 1)
            row["share_of_bf16_peak"] = round(flops[k] / (med[k] * 1e-3) / PEAK_BF16_FLOPS, 4)
        print(json.dumps(row), flush=True)
    return med


def random_net(seed=0):
    """He-scaled convolutions, non-trivial BatchNorm statistics (the numbers do not matter for the timing, NaNs would)"""
    g = torch.Generator().manual_seed(seed)
    net = MedicalNetResNet10()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.Conv3d):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) * math.sqrt(2.0 / m.weight[0].numel()))
            elif isinstance(m, torch.nn.BatchNorm3d):
                m.running_var.copy_(0.5 + 1.5 * torch.rand(m.num_features, generator=g))
                m.running_mean.copy_(0.1 * torch.randn(m.num_features, generator=g))
    return net.cuda()


def out_extent(n, stride):
    return (n - 1) // stride + 1


def conv_flops(samples, size):
    """name -> FLOPs (2 per multiply-add, the algorithm's own K: 343 for the stem) of every convolution, from the shapes"""
    f, s = {}, out_extent(size, 2)
    f["stem"] = 2.0 * samples * s ** 3 * 343 * 64
    s = out_extent(s, 2)
    for name, cin, cout, stride, _dil in BLOCKS:
        so = out_extent(s, stride)
        vox = samples * so ** 3
        f[name] = 2.0 * vox * 27 * cin * cout + 2.0 * vox * 27 * cout * cout + (2.0 * vox * cin * cout if (stride != 1 or cin != cout) else 0.0)
        s = so
    return f


def bench_ours(net, pred, target, reps):
    term = PerceptualLoss(net)
    b, c = pred.shape[:2]
    samples = b * c
    flops = conv_flops(samples, pred.shape[2])
    p = net.packed()
    vols = pred.view(samples, *pred.shape[2:])
    ms = ops.medicalnet_moments(pred)
    stem = ops.medicalnet_stem(vols, ms, p["stem.w"], p["stem.b"])
    a = ops.medicalnet_maxpool(stem)
    fns = {"perceptual_forward": lambda: term(pred, target), "extractor_one_tensor": lambda: net.features(pred),
           "moments": lambda: ops.medicalnet_moments(pred),
           "stem": lambda: ops.medicalnet_stem(vols, ms, p["stem.w"], p["stem.b"]), "maxpool": lambda: ops.medicalnet_maxpool(stem)}
    for name, _cin, cout, stride, dil in BLOCKS:
        def block(a=a, name=name, cout=cout, stride=stride, dil=dil):
            t = ops.medicalnet_conv(a, p[f"{name}.conv1.w"], p[f"{name}.conv1.b"], cout, 3, stride, dil)
            r = a
            if f"{name}.down.w" in p:
                r = ops.medicalnet_conv(a, p[f"{name}.down.w"], p[f"{name}.down.b"], cout, 1, stride, 1, relu=False)
            return ops.medicalnet_conv(t, p[f"{name}.conv2.w"], p[f"{name}.conv2.b"], cout, 3, 1, dil, residual=r)
        fns[name] = block
        a = block()
    fp, ft = a, net.features(target)
    fns["tail"] = lambda: ops.medicalnet_tail(fp, ft, b, c)
    total = sum(flops.values())
    flops.update(perceptual_forward=2 * total, extractor_one_tensor=total)
    return report("hip", rounds(fns, reps), flops)


def bench_stock(net, pred, reps):
    """the same network as stock torch modules in bf16, channels-last, on the normalised tensor (normalisation not timed)"""
    m = copy.deepcopy(net).to(torch.bfloat16).to(memory_format=torch.channels_last_3d)
    x = ((pred - pred.mean()) / pred.std()).view(-1, 1, *pred.shape[2:]).to(torch.bfloat16).contiguous(memory_format=torch.channels_last_3d)

    def stem(x):
        return F.relu(m.bn1(m.conv1(x)))

    def block(blk, x):
        out = blk.bn2(blk.conv2(F.relu(blk.bn1(blk.conv1(x)))))
        return F.relu(out + (x if blk.downsample is None else blk.downsample(x)))

    with torch.no_grad():
        s = stem(x)
        a = F.max_pool3d(s, 3, 2, 1)
        fns = {"stem": lambda: stem(x), "maxpool": lambda: F.max_pool3d(s, 3, 2, 1)}
        chain = [a]
        for name, *_ in BLOCKS:
            blk = getattr(m, name)[0]
            fns[name] = lambda blk=blk, a=chain[-1]: block(blk, a)
            chain.append(block(blk, chain[-1]))

        def whole():
            a = F.max_pool3d(stem(x), 3, 2, 1)
            for name, *_ in BLOCKS:
                a = block(getattr(m, name)[0], a)
            return a
        fns["extractor_one_tensor"] = whole
        flops = conv_flops(x.shape[0], x.shape[2])
        flops["extractor_one_tensor"] = sum(flops.values())
        return report("stock_torch_bf16", rounds(fns, reps, warmup=2), flops)


def bench_backward(net, pred, target, reps):
    """the differentiable term: forward with the activations kept, backward whole and by part"""
    b, c = pred.shape[:2]
    samples = b * c
    flops = conv_flops(samples, pred.shape[2])
    p = net.packed()
    term = PerceptualLoss(net, differentiable=True, factor=1e3)
    leaf = pred.clone().requires_grad_()
    up = torch.ones((), device=pred.device)
    kept = {}
    fp, ft = net.features(pred, keep=kept), net.features(target)
    g_out = torch.full((1,), 1e3, device=pred.device)
    vols = pred.view(samples, *pred.shape[2:])
    holder = {}

    def fwd_bwd():
        torch.autograd.grad(term(leaf, target), leaf, up)

    def backward_only():
        if "v" not in holder:
            holder["v"] = term(leaf, target)
        torch.autograd.grad(holder["v"], leaf, up, retain_graph=True)

    def whole():
        return medicalnet_backward(net, pred, kept, ops.medicalnet_tail_bwd(fp, ft, g_out, b, c))
    fns = {"forward_keep_plus_backward": fwd_bwd, "backward": backward_only, "backward_launches": whole,
           "tail_bwd": lambda: ops.medicalnet_tail_bwd(fp, ft, g_out, b, c)}
    g = ops.medicalnet_tail_bwd(fp, ft, g_out, b, c)
    inputs = (kept["pool"],) + tuple(kept[f"{name}.out"] for name, *_ in BLOCKS[:-1])
    for k in range(len(BLOCKS) - 1, -1, -1):
        name, _cin, _cout, stride, dil = BLOCKS[k]

        def block(g=g, name=name, stride=stride, dil=dil, a_in=inputs[k], k=k):
            g_t = ops.medicalnet_dgrad(g, p[f"{name}.conv2.dw"], kept[f"{name}.t"].shape, 3, 1, dil, mask=kept[f"{name}.t"])
            r = ops.medicalnet_dgrad(g, p[f"{name}.down.dw"], a_in.shape, 1, stride, 1) if f"{name}.down.dw" in p else g
            return ops.medicalnet_dgrad(g_t, p[f"{name}.conv1.dw"], a_in.shape, 3, stride, dil, add=r, mask=a_in if k > 0 else None)
        fns[name + "_bwd"] = block
        flops[name + "_bwd"] = flops[name]
        g = block()
    g_pool = g
    g_stem = ops.medicalnet_maxpool_bwd(kept["stem"], g_pool)
    g_hat, part = ops.medicalnet_stem_dgrad(g_stem, p["stem.dw"], vols, kept["mean_std"])
    fns["maxpool_bwd"] = lambda: ops.medicalnet_maxpool_bwd(kept["stem"], g_pool)
    fns["stem_bwd"] = lambda: ops.medicalnet_stem_dgrad(g_stem, p["stem.dw"], vols, kept["mean_std"])
    fns["norm_bwd"] = lambda: ops.medicalnet_norm_bwd(g_hat, vols, kept["mean_std"], part)
    flops["stem_bwd"] = flops["stem"]
    total = sum(flops[k] for k in ("stem",) + tuple(n for n, *_ in BLOCKS))
    flops.update(backward=total, backward_launches=total, forward_keep_plus_backward=3 * total)
    return report("hip_backward", rounds(fns, reps), flops)


def bench_stock_backward(net, pred, reps):
    """the same network's backward with respect to its input as stock torch autograd, bf16, channels-last, part by part"""
    m = copy.deepcopy(net).to(torch.bfloat16).to(memory_format=torch.channels_last_3d)
    x = ((pred - pred.mean()) / pred.std()).view(-1, 1, *pred.shape[2:]).to(torch.bfloat16).contiguous(memory_format=torch.channels_last_3d)

    def stem(x):
        return F.relu(m.bn1(m.conv1(x)))

    def block(blk, x):
        out = blk.bn2(blk.conv2(F.relu(blk.bn1(blk.conv1(x)))))
        return F.relu(out + (x if blk.downsample is None else blk.downsample(x)))

    def part(fn, x):
        """backward of one part alone: its forward graph is built once and kept"""
        leaf = x.detach().clone().requires_grad_()
        y = fn(leaf)
        gy = torch.randn_like(y)
        return y.detach(), (lambda: torch.autograd.grad(y, leaf, gy, retain_graph=True))
    fns = {}
    s, fns["stem_bwd"] = part(stem, x)
    a, fns["maxpool_bwd"] = part(lambda t: F.max_pool3d(t, 3, 2, 1), s)
    for name, *_ in BLOCKS:
        a, fns[name + "_bwd"] = part(lambda t, blk=getattr(m, name)[0]: block(blk, t), a)

    def whole(t):
        t = F.max_pool3d(stem(t), 3, 2, 1)
        for name, *_ in BLOCKS:
            t = block(getattr(m, name)[0], t)
        return t
    _, fns["backward"] = part(whole, x)
    flops = conv_flops(x.shape[0], x.shape[2])
    flops = {k + "_bwd": v for k, v in flops.items()}
    flops["backward"] = sum(flops.values())
    return report("stock_torch_bf16_backward", rounds(fns, reps, warmup=2), flops)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="ours,stock")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--channels", type=int, default=6)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--lib", default=None, help="another build of the C ABI, e.g. the parent commit's, for an interleaved A/B")
    a = ap.parse_args()
    if a.lib:
        import tools.diaglib as D
        D.use(a.lib)
    assert torch.cuda.is_available(), "this tool measures on the GPU"
    g = torch.Generator().manual_seed(3)
    shape = (a.batch, a.channels, a.size, a.size, a.size)
    target = torch.rand(shape, generator=g)
    pred = (target + 0.2 * torch.randn(shape, generator=g)).cuda()
    target = target.cuda()
    net = random_net()
    print(json.dumps(dict(what="shape", pred=list(shape), samples_per_tensor=a.batch * a.channels, lib=a.lib)), flush=True)
    parts = a.parts.split(",")
    ours = stock = None
    if "ours" in parts:
        ours = bench_ours(net, pred, target, a.reps)
    if "stock" in parts:
        stock = bench_stock(net, pred, a.reps)
    if ours and stock:
        keys = [k for k in stock if k in ours]
        print(json.dumps(dict(what="hip_over_stock", **{k: round(ours[k] / stock[k], 3) for k in keys})), flush=True)
    ours = stock = None
    if "backward" in parts:
        ours = bench_backward(net, pred, target, a.reps)
    if "stock_backward" in parts:
        stock = bench_stock_backward(net, pred, a.reps)
    if ours and stock:
        keys = [k for k in stock if k in ours]
        print(json.dumps(dict(what="hip_over_stock_backward", **{k: round(ours[k] / stock[k], 3) for k in keys})), flush=True)
