"""Index-level references of the row kernels that only move or pick data (csrc/layout_pack.hip, csrc/pool.hip,
csrc/fp8_prep.hip), for tests/test_row_kernels_gpu.py and their CPU self-tests (tests/test_row_kernels_ref.py).

A correct kernel is bit-identical to these: plain torch on the CPU, no tolerance anywhere.  Comparisons go through
``same_bits`` (bit views; a NaN is compared as a position, its payload and sign are not) and, for e4m3 bytes, ``fold_nan``.
"""
import torch

_BITS = {4: torch.int32, 2: torch.int16, 1: torch.uint8}
SCAN = [(kd, kh, kw) for kd in (0, 1) for kh in (0, 1) for kw in (0, 1)]      # window position k = 4 kd + 2 kh + kw


def bits(t):
    return t.contiguous().view(_BITS[t.element_size()])


def same_bits(got, want):
    """NaN at the same positions, every other element bit-identical (+0 and -0 differ)."""
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if not got.dtype.is_floating_point:
        return torch.equal(got, want)
    gn, wn = got.isnan(), want.isnan()
    zero = torch.zeros((), dtype=got.dtype)
    return torch.equal(gn, wn) and torch.equal(bits(torch.where(gn, zero, got)), bits(torch.where(wn, zero, want)))


def fold_nan(b):
    """e4m3 bytes with both NaN encodings (0x7f, 0xff) folded to 0x7f: the sign bit of a NaN byte is not compared."""
    return torch.where((b & 0x7F) == 0x7F, torch.full((), 0x7F, dtype=torch.uint8), b)


# ------------------------------------------------------------------------------------------------------------- layout
def s2d_cells(a):
    """Plain NDHWC tensor (n, d, h, w, c), even extents -> its space-to-depth cells (n, d/2+1, h/2+1, w/2+1, 8, c) from the
    definition S(a)[j, blk] = a[2 j + b - 1] on the zero-padded volume, blk = 4 bd + 2 bh + bw."""
    n, d, h, w, c = a.shape
    xp = torch.zeros(n, d + 2, h + 2, w + 2, c, dtype=a.dtype)
    xp[:, 1:-1, 1:-1, 1:-1] = a
    return torch.stack([xp[:, bd::2, bh::2, bw::2] for bd, bh, bw in SCAN], 4)


def pack_ref(srcs, dtype, ld, coff, zero_to, s2d_cblk=0):
    """mi355_pack_ncdhw / pack2 (two sources) / their _s2d forms: the NCDHW f32 sources, concatenated along channels, permuted
    to rows, rounded through `dtype`, placed at [coff, coff + c) with zeros up to zero_to.  Returns (val, mask): the destination
    (rows of ld elements) with zeros where nothing is written, and the elements the kernel is allowed to write -- in the
    space-to-depth form every block's window, the zero blocks of the border cells included."""
    x = torch.cat(list(srcs), 1)
    n, c, d, h, w = x.shape
    wch = zero_to - coff
    win = torch.zeros(n, d, h, w, wch, dtype=dtype)
    win[..., :c] = x.permute(0, 2, 3, 4, 1).to(dtype)
    if not s2d_cblk:
        val = torch.zeros(n, d, h, w, ld, dtype=dtype)
        mask = torch.zeros(val.shape, dtype=torch.bool)
        val[..., coff:zero_to] = win
        mask[..., coff:zero_to] = True
        return val, mask
    cells = s2d_cells(win)
    val = torch.zeros(*cells.shape[:4], ld, dtype=dtype)
    mask = torch.zeros(val.shape, dtype=torch.bool)
    for blk in range(8):
        val[..., blk * s2d_cblk + coff: blk * s2d_cblk + zero_to] = cells[..., blk, :]
        mask[..., blk * s2d_cblk + coff: blk * s2d_cblk + zero_to] = True
    return val, mask


def written(before, val, mask):
    """The destination after a pack: the reference where the kernel may write, the earlier content everywhere else."""
    return torch.where(mask, val, before)


def unpack_ref(src, c, coff, s2d=None):
    """mi355_unpack_ncdhw(_s2d): channels [coff, coff + c) of the rows (s2d = (d, h, w, cblk): of the blocks of S) as NCDHW f32."""
    if s2d is None:
        return src[..., coff:coff + c].float().permute(0, 4, 1, 2, 3).contiguous()
    d, h, w, cblk = s2d
    i, j, k = torch.arange(d).view(-1, 1, 1), torch.arange(h).view(1, -1, 1), torch.arange(w).view(1, 1, -1)
    blk = ((i + 1) & 1) * 4 + ((j + 1) & 1) * 2 + ((k + 1) & 1)                  # a[i] = S[(i + 1) >> 1, b = (i + 1) & 1]
    ch = blk[..., None] * cblk + coff + torch.arange(c)
    rows = src[:, ((i + 1) >> 1)[..., None], ((j + 1) >> 1)[..., None], ((k + 1) >> 1)[..., None], ch]
    return rows.float().permute(0, 4, 1, 2, 3).contiguous()


# ------------------------------------------------------------------------------------------------------------- max-pool
def _windows(x):
    n, d, h, w, c = x.shape
    od, oh, ow = d // 2, h // 2, w // 2
    return torch.stack([x[:, kd:2 * od:2, kh:2 * oh:2, kw:2 * ow:2] for kd, kh, kw in SCAN])


def _first(flag):
    """Index of the first True along axis 0 (0 where there is none)."""
    first = flag & (flag.cumsum(0) == 1)
    return (first * torch.arange(flag.shape[0]).view(-1, *([1] * (flag.dim() - 1)))).sum(0)


class PoolRef:
    pass


def pool_ref(x, dy=None, add=None):
    """MaxPool3d(2) of NDHWC rows (n, d, h, w, c), f32 or bf16, floor mode.  The 8 window elements in scan order (kd, kh, kw):
    y is NaN if the window holds one, else the maximum; `where` is the first NaN in scan order if there is one, else the first
    element equal to the maximum (y carries that element's bits: -0 before +0 gives -0, as F.max_pool3d's strict `>` scan
    does); dx routes dy to `where`, voxels outside every window get 0; `add` is then summed in f32 and rounded once."""
    r = PoolRef()
    w8 = _windows(x.float())
    isn = w8.isnan()
    r.nans = isn.sum(0)
    wm = torch.where(isn, torch.full((), float("-inf")), w8)
    mx = wm.max(0).values
    r.where = torch.where(r.nans > 0, _first(isn), _first(wm == mx))
    picked = w8.gather(0, r.where[None])[0]
    r.y = torch.where(r.nans > 0, torch.full((), float("nan")), picked).to(x.dtype)
    r.where = r.where.to(torch.uint8)
    if dy is None:
        return r
    n, d, h, w, c = x.shape
    od, oh, ow = d // 2, h // 2, w // 2
    dx = torch.zeros(n, d, h, w, c)
    for k, (kd, kh, kw) in enumerate(SCAN):
        dx[:, kd:2 * od:2, kh:2 * oh:2, kw:2 * ow:2] = torch.where(r.where == k, dy.float(), torch.zeros(()))
    r.dx = dx.to(x.dtype)
    r.dx_add = None if add is None else (dx + add.float()).to(x.dtype)
    return r


def pool_case(n, dims, c, seed):
    """Input of the max-pool tests, f32 (every value exact in bf16): integers in [-2, 2] (ties in most windows) and, in
    (window, channel) slots spread over the tensor: +0 against -0 in either order, an all -inf window, a +inf, one NaN at each
    of the 8 positions, two NaNs, eight NaNs.  Returns (x, special): special[slot name] = flat (window, channel) index."""
    g = torch.Generator().manual_seed(seed)
    d, h, w = dims
    od, oh, ow = d // 2, h // 2, w // 2
    x = torch.randint(-2, 3, (n, d, h, w, c), generator=g).float()
    w8 = _windows(x).reshape(8, -1).clone()
    slots = w8.shape[1]
    names = ["zero_neg_first", "zero_pos_first", "all_neg_inf", "pos_inf"] + [f"nan_at_{k}" for k in range(8)] + ["two_nans", "eight_nans"]
    assert slots >= len(names)
    step = slots // len(names)
    special = {}
    nan, inf = float("nan"), float("inf")
    for i, name in enumerate(names):
        s = i * step
        special[name] = s
        if name.startswith("zero"):
            w8[:, s] = -1.0
            w8[2, s], w8[5, s] = (-0.0, 0.0) if name == "zero_neg_first" else (0.0, -0.0)
        elif name == "all_neg_inf":
            w8[:, s] = -inf
        elif name == "pos_inf":
            w8[6, s] = inf
        elif name.startswith("nan_at_"):
            w8[int(name[-1]), s] = nan
        elif name == "two_nans":
            w8[3, s] = w8[6, s] = nan
        else:
            w8[:, s] = nan
    w8 = w8.view(8, n, od, oh, ow, c)
    for k, (kd, kh, kw) in enumerate(SCAN):
        x[:, kd:2 * od:2, kh:2 * oh:2, kw:2 * ow:2] = w8[k]
    return x, special


# ------------------------------------------------------------------------------------------------------------- fp8 preparation
def e4m3_ref(x_f32, amax):
    """mi355_cast_fp8: the e4m3 bytes of x * (224 / amax) (f32 arithmetic; scale 1 when amax is 0), saturated at +-448, NaN kept."""
    a = torch.tensor(float(amax), dtype=torch.float32)
    sc = torch.tensor(224.0, dtype=torch.float32) / a if float(amax) > 0 else torch.tensor(1.0)
    return (x_f32 * sc).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)


def amax_ref(x):
    """max |x| as the kernels form it: fmaxf from 0 drops NaN, keeps inf."""
    a = x.float().abs()
    return torch.where(a.isnan(), torch.zeros(()), a).max()


def scale_roll_ref(table, n, sat=None):
    """mi355_fp8_scale_roll on the first n rows of table [rows][2] = (in use, gathered); sat (int32) counts the slots that clamped."""
    table = table.clone()
    use, nx = table[:n, 0].clone(), table[:n, 1].clone()
    if sat is not None:
        sat = sat.clone()
        sat[:n] += ((use > 0) & (nx > 2.0 * use)).to(torch.int32)
    table[:n, 0] = torch.where(nx > 0, nx, use)
    table[:n, 1] = 0.0
    return table, sat


def e4m3_values():
    """The 254 finite e4m3 values (both zeros), ascending by value."""
    b = torch.arange(256, dtype=torch.uint8)
    v = b.view(torch.float8_e4m3fn).float()
    return v[~v.isnan()].sort().values


def e4m3_rounding_probe():
    """f32 inputs that pin round-to-nearest-even and the subnormal range at scale 1: every finite e4m3 value, the midpoint between
    every pair of neighbours, and the two f32 neighbours of each of those."""
    v = torch.unique(e4m3_values())                                  # +0 and -0 collapse
    mid = (v[:-1] + v[1:]) / 2                                        # exact in f32: neighbours differ by one e4m3 ulp
    base = torch.cat([v, torch.tensor([-0.0]), mid])
    up = torch.nextafter(base, torch.full_like(base, float("inf")))
    down = torch.nextafter(base, torch.full_like(base, float("-inf")))
    return torch.cat([base, up, down])
