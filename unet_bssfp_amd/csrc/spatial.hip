// Spatial augmentation (tio.RandomFlip, tio.RandomAffine) fused into the patch gather:
//     out_j[b][ch][z][y][x] = A_b( Tens_{l,j}( trilinear( P(src_j), M_l (o_b + (z, y, x), 1) ) ) )
// P (crop/pad by index arithmetic), o_b and the fused stages A_b are those of patch_queue.hip; the coordinate arithmetic,
// the inside test and the clamped corners are those of motion.hip's resampler (resample_core.h), taken in the padded
// volume's coordinates.  A corner that lands on a pad voxel of P reads the padding value; neither the padded nor the
// resampled volume exists in HBM.  Bias coordinates and noise keys come from the output position, as if the resampled
// volume had been materialised first, so a patch equals extract_patches(chain(affine_resample(crop_or_pad(raw)))) bit for
// bit, and affine_resample is this launch with one patch that is the volume.
//
// One lane owns VEC = 4 consecutive output voxels of a patch row (VEC = 1 when pw % 4 != 0 or an output is not 16-byte
// aligned).  Where each voxel reads -- inside or not, four row offsets, two columns, three weights -- is computed once and
// reused by every channel.  A voxel whose three weights are 0 (every voxel of a flip: (T - 1) - i is exact in f32) reads
// its one source voxel instead of eight, so a flip costs index arithmetic only; lerp(a, b, 0) = a, so this changes no value.
// A tensor image (6 channels dxx, dxy, dxz, dyy, dyz, dzz) samples its six channels first and maps every inside voxel
// through the load's 6 x 6 matrix and 6-vector: six fmas per component, j in order, starting from the vector's entry.
// Descriptors travel by value in the kernel arguments: no atomics, no scratch, no workspace, no host synchronisation.
#include "common.h"
#include "augment_core.h"
#include "resample_core.h"

namespace {

struct SSrc {
  const float* src; const double* cmin;   // cmin: null, or (sum, min) pairs per channel
  int d, h, w, sz, sy, sx;                // raw = padded + (sz, sy, sx)
  float fill; int resample;
};
struct SImg { float* dst; int c, aug, tensor; };                     // dst = patch 0 of the chunk
struct SArgs {
  mi355_queue_load load[MI355_QUEUE_MAX_LOADS];
  mi355_queue_spatial sp[MI355_QUEUE_MAX_LOADS];
  SSrc src[MI355_QUEUE_MAX_LOADS][MI355_QUEUE_MAX_IMAGES];
  SImg img[MI355_QUEUE_MAX_IMAGES];
  int patch[MI355_MAX_PATCHES][4];                                   // local load slot, origin z, y, x (padded)
  int td, th, tw, pd, ph, pw;
  float pad;
};
static_assert(sizeof(SArgs) <= 4096, "the descriptors of a chunk must fit the kernel argument block");

// where one output voxel reads in the RAW volume: row[a][b] = offset of the row (corner a along D, b along H) inside a
// channel, col[c] = the column; -1 = a pad voxel of P.  near: the three weights are 0 and corner (0, 0, 0) is the value.
struct Tap {
  int row[2][2], col[2];
  float t0, t1, t2;
  bool inside, near;
};

__device__ __forceinline__ int raw_index(int padded, int shift, int n) {
  const int r = padded + shift;
  return r >= 0 && r < n ? r : -1;
}

__device__ __forceinline__ Tap make_tap(const SSrc& S, const Rigid& q, int td, int th, int tw, int pz, int py, int px) {
  Tap t;
  int z[2], y[2], x[2];
  if (S.resample) {
    const ResamplePoint p = resample_point(q, td, th, tw, pz, py, px);
    t.inside = p.inside;
    t.t0 = p.t0; t.t1 = p.t1; t.t2 = p.t2;
    t.near = p.t0 == 0.f && p.t1 == 0.f && p.t2 == 0.f;
    z[0] = p.lo0; z[1] = p.hi0; y[0] = p.lo1; y[1] = p.hi1; x[0] = p.lo2; x[1] = p.hi2;
  } else {
    t.inside = true; t.near = true;
    t.t0 = t.t1 = t.t2 = 0.f;
    z[0] = z[1] = pz; y[0] = y[1] = py; x[0] = x[1] = px;
  }
#pragma unroll
  for (int a = 0; a < 2; ++a) {
    const int rz = t.inside ? raw_index(z[a], S.sz, S.d) : -1;       // an outside point gathers nothing
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int ry = raw_index(y[b], S.sy, S.h);
      t.row[a][b] = rz >= 0 && ry >= 0 ? (rz * S.h + ry) * S.w : -1;
    }
    t.col[a] = raw_index(x[a], S.sx, S.w);
  }
  return t;
}

__device__ __forceinline__ float fetch(const float* __restrict__ xc, int row, int col, float pad) {
  return row >= 0 && col >= 0 ? xc[row + col] : pad;
}

__device__ __forceinline__ float tap_value(const float* __restrict__ xc, const Tap& t, float pad, float fill) {
  if (!t.inside) return fill;
  if (t.near) return fetch(xc, t.row[0][0], t.col[0], pad);
  float v[2][2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int c = 0; c < 2; ++c) v[a][b][c] = fetch(xc, t.row[a][b], t.col[c], pad);
  return trilinear(v, t.t0, t.t1, t.t2);
}

// G channels at a time: 6 with the tensor map (the whole image), else 2 (their gathers in flight together)
template <int VEC, int G, bool TENSOR>
__device__ __forceinline__ void walk_channels(const SArgs& A, const SSrc& S, const SImg& I, const mi355_queue_load& L,
                                              const mi355_queue_spatial& sp, const Tap (&tap)[VEC], const float (&g)[VEC],
                                              int ns, long long flat0, float* __restrict__ dst) {
  const long long svol = (long long)S.d * S.h * S.w;
  const long long pv = (long long)A.pd * A.ph * A.pw;
  const long long tvol = (long long)A.td * A.th * A.tw;
  for (int c0 = 0; c0 < I.c; c0 += G) {
    float v[G][VEC];
#pragma unroll
    for (int u = 0; u < G; ++u) {
      const int ch = c0 + u;
      if (ch < I.c) {
        const float fill = S.cmin ? (float)S.cmin[2 * ch + 1] : S.fill;
#pragma unroll
        for (int k = 0; k < VEC; ++k) v[u][k] = tap_value(S.src + ch * svol, tap[k], A.pad, fill);
      }
    }
    if constexpr (TENSOR) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        if (!tap[k].inside) continue;                                // the fill is not mapped
        float n[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
          float acc = sp.t6[36 + i];
#pragma unroll
          for (int j = 0; j < 6; ++j) acc = fmaf(sp.t6[6 * i + j], v[j][k], acc);
          n[i] = acc;
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) v[i][k] = n[i];
      }
    }
#pragma unroll
    for (int u = 0; u < G; ++u) {
      const int ch = c0 + u;
      if (ch >= I.c) break;
      for (int s = 0; s < ns; ++s) {
        const int kind = L.stage[s];
        if (kind == MI355_STAGE_BIAS_FIELD) {
#pragma unroll
          for (int k = 0; k < VEC; ++k) v[u][k] = aug_bias_apply(v[u][k], g[k]);
        } else if (kind == MI355_STAGE_NOISE) {
#pragma unroll
          for (int k = 0; k < VEC; ++k) v[u][k] = aug_noise_apply(v[u][k], ch * tvol + flat0 + k, L.noise_mean, L.noise_std, L.noise_seed);
        } else {
#pragma unroll
          for (int k = 0; k < VEC; ++k) v[u][k] = aug_gamma_apply(v[u][k], L.gamma);
        }
      }
      float* o = dst + ch * pv;
      if constexpr (VEC == 4) {
        f32x4 t;
        t[0] = v[u][0]; t[1] = v[u][1]; t[2] = v[u][2]; t[3] = v[u][3];
        *reinterpret_cast<f32x4*>(o) = t;
      } else {
        o[0] = v[u][0];
      }
    }
  }
}

// grid: (runs of a patch / 256, patches of the chunk, images)
template <int VEC>
__global__ __launch_bounds__(256) void spatial_queue_kernel(const SArgs A) {
  const int b = blockIdx.y, j = blockIdx.z;
  const int wv = A.pw / VEC;
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= (long long)A.pd * A.ph * wv) return;
  const int z = (int)(r / ((long long)A.ph * wv)), y = (int)(r / wv % A.ph), x = (int)(r % wv) * VEC;
  const int l = A.patch[b][0];
  const int pz = A.patch[b][1] + z, py = A.patch[b][2] + y, px = A.patch[b][3] + x;   // padded coordinates
  const SSrc& S = A.src[l][j];
  const SImg& I = A.img[j];
  const mi355_queue_load& L = A.load[l];
  const mi355_queue_spatial& sp = A.sp[l];
  const long long pv = (long long)A.pd * A.ph * A.pw;
  float* __restrict__ dst = I.dst + (long long)b * I.c * pv + ((long long)z * A.ph + y) * A.pw + x;
  const int ns = I.aug ? L.nstages : 0;
  const long long flat0 = ((long long)pz * A.th + py) * A.tw + px;                       // noise key of channel 0

  Rigid q;
#pragma unroll
  for (int i = 0; i < 12; ++i) q.m[i] = sp.m[i];
  Tap tap[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) tap[k] = make_tap(S, q, A.td, A.th, A.tw, pz, py, px + k);

  float g[VEC];                                                                           // bias field: position only
#pragma unroll
  for (int k = 0; k < VEC; ++k) g[k] = 1.f;
  bool bias = false;
  for (int s = 0; s < ns; ++s) bias |= L.stage[s] == MI355_STAGE_BIAS_FIELD;
  if (bias) {
#pragma unroll
    for (int k = 0; k < VEC; ++k)
      g[k] = expf(aug_bias_log_field(pz, py, px + k, A.td, A.th, A.tw, L.bias_order, L.bias_coef));
  }

  if (I.tensor && S.resample) walk_channels<VEC, 6, true>(A, S, I, L, sp, tap, g, ns, flat0, dst);
  else walk_channels<VEC, 2, false>(A, S, I, L, sp, tap, g, ns, flat0, dst);
}

// raw coordinate = padded coordinate + shift: augment.crop_or_pad's centred crop ((n - t) // 2 dropped before) or pad
// ((t - n) // 2 added before)
int crop_pad_shift(int n, int t) { return n > t ? (n - t) / 2 : -((t - n) / 2); }

bool finite(float v) { return v == v && v - v == 0.f; }

}  // namespace

extern "C" int mi355_patch_queue_gather_spatial(const mi355_queue_load* loads, const mi355_queue_spatial* spatial,
                                                int32_t nloads, const mi355_queue_source* sources,
                                                const mi355_queue_resampling* resampling, const int32_t* channels,
                                                const int32_t* augmented, const int32_t* tensor, float* const* outs,
                                                int32_t nimages, const int32_t* patches, int32_t npatches, int32_t td,
                                                int32_t th, int32_t tw, int32_t pd, int32_t ph, int32_t pw,
                                                float padding_value, void* stream) {
  MI355_REQUIRE(npatches >= 0, "patch_queue_gather_spatial: bad patch count");
  MI355_REQUIRE(td > 0 && th > 0 && tw > 0 && pd > 0 && ph > 0 && pw > 0 && pd <= td && ph <= th && pw <= tw,
                "patch_queue_gather_spatial: bad patch (%d, %d, %d) or target (%d, %d, %d) shape", pd, ph, pw, td, th, tw);
  MI355_REQUIRE((long long)td * th * tw < (1LL << 31), "patch_queue_gather_spatial: target volume too large");
  MI355_REQUIRE(nimages > 0 && nimages <= MI355_QUEUE_MAX_IMAGES, "patch_queue_gather_spatial: 1..%d images, got %d",
                MI355_QUEUE_MAX_IMAGES, nimages);
  if (npatches == 0) return MI355_OK;
  MI355_REQUIRE(loads && spatial && sources && resampling && channels && augmented && tensor && outs && patches,
                "patch_queue_gather_spatial: null pointer");
  MI355_REQUIRE(nloads > 0, "patch_queue_gather_spatial: no subject load");
  for (int l = 0; l < nloads; ++l) {
    const mi355_queue_load& L = loads[l];
    MI355_REQUIRE(L.nstages >= 0 && L.nstages <= MI355_QUEUE_MAX_STAGES, "patch_queue_gather_spatial: load %d: bad stage count", l);
    int seen = 0;
    for (int s = 0; s < L.nstages; ++s) {
      const int k = L.stage[s];
      MI355_REQUIRE(k >= MI355_STAGE_BIAS_FIELD && k <= MI355_STAGE_GAMMA && !(seen & (1 << k)),
                    "patch_queue_gather_spatial: load %d: bad or repeated stage %d", l, k);
      seen |= 1 << k;
    }
    MI355_REQUIRE(L.bias_order >= 0 && L.bias_order <= 4, "patch_queue_gather_spatial: load %d: bias order must be 0..4", l);
    MI355_REQUIRE(L.noise_std >= 0.f, "patch_queue_gather_spatial: load %d: negative noise std", l);
    bool any = false;
    for (int j = 0; j < nimages; ++j) {
      const mi355_queue_source& s = sources[(long long)l * nimages + j];
      MI355_REQUIRE(s.src && s.d > 0 && s.h > 0 && s.w > 0, "patch_queue_gather_spatial: load %d image %d: bad source", l, j);
      MI355_REQUIRE((long long)s.d * s.h * s.w < (1LL << 31), "patch_queue_gather_spatial: load %d image %d: source too large", l, j);
      const mi355_queue_resampling& rs = resampling[(long long)l * nimages + j];
      any = any || rs.resample;
      MI355_REQUIRE(!rs.resample || rs.channel_min || finite(rs.fill), "patch_queue_gather_spatial: load %d image %d: fill is not finite", l, j);
    }
    if (any)
      for (int i = 0; i < 54; ++i)
        MI355_REQUIRE(finite(i < 12 ? spatial[l].m[i] : spatial[l].t6[i - 12]),
                      "patch_queue_gather_spatial: load %d: matrix entry %d is not finite", l, i);
  }
  bool vec = pw % 4 == 0;
  for (int j = 0; j < nimages; ++j) {
    MI355_REQUIRE(outs[j] && channels[j] > 0 && channels[j] <= 65535, "patch_queue_gather_spatial: image %d: bad output", j);
    MI355_REQUIRE(!tensor[j] || channels[j] == 6, "patch_queue_gather_spatial: image %d: a tensor image has 6 channels, got %d", j, channels[j]);
    vec = vec && ((uintptr_t)outs[j] & 15) == 0;
  }
  for (int b = 0; b < npatches; ++b) {
    const int32_t* p = patches + 4LL * b;
    MI355_REQUIRE(p[0] >= 0 && p[0] < nloads, "patch_queue_gather_spatial: patch %d: load %d out of range", b, p[0]);
    MI355_REQUIRE(p[1] >= 0 && p[1] + pd <= td && p[2] >= 0 && p[2] + ph <= th && p[3] >= 0 && p[3] + pw <= tw,
                  "patch_queue_gather_spatial: patch %d leaves the target volume", b);
  }
  const long long pv = (long long)pd * ph * pw;
  const long long runs = pv / (vec ? 4 : 1);
  MI355_REQUIRE((runs + 255) / 256 < (1LL << 31), "patch_queue_gather_spatial: patch too large");
  for (int b0 = 0; b0 < npatches;) {
    // a chunk: at most MI355_MAX_PATCHES patches of at most MI355_QUEUE_MAX_LOADS distinct loads
    SArgs A;
    int slot_of[MI355_QUEUE_MAX_LOADS], nslots = 0, n = 0;
    while (b0 + n < npatches && n < MI355_MAX_PATCHES) {
      const int32_t* p = patches + 4LL * (b0 + n);
      int s = 0;
      while (s < nslots && slot_of[s] != p[0]) ++s;
      if (s == nslots) {
        if (nslots == MI355_QUEUE_MAX_LOADS) break;
        slot_of[nslots++] = p[0];
      }
      A.patch[n][0] = s; A.patch[n][1] = p[1]; A.patch[n][2] = p[2]; A.patch[n][3] = p[3];
      ++n;
    }
    for (int s = 0; s < nslots; ++s) {
      A.load[s] = loads[slot_of[s]];
      A.sp[s] = spatial[slot_of[s]];
      for (int j = 0; j < nimages; ++j) {
        const mi355_queue_source& src = sources[(long long)slot_of[s] * nimages + j];
        const mi355_queue_resampling& rs = resampling[(long long)slot_of[s] * nimages + j];
        A.src[s][j] = SSrc{src.src, rs.channel_min, src.d, src.h, src.w, crop_pad_shift(src.d, td), crop_pad_shift(src.h, th),
                           crop_pad_shift(src.w, tw), rs.fill, rs.resample != 0};
      }
    }
    for (int j = 0; j < nimages; ++j)
      A.img[j] = SImg{outs[j] + (long long)b0 * channels[j] * pv, channels[j], augmented[j] != 0, tensor[j] != 0};
    A.td = td; A.th = th; A.tw = tw; A.pd = pd; A.ph = ph; A.pw = pw; A.pad = padding_value;
    const dim3 grid((unsigned)((runs + 255) / 256), n, nimages);
    if (vec) spatial_queue_kernel<4><<<grid, 256, 0, (hipStream_t)stream>>>(A);
    else spatial_queue_kernel<1><<<grid, 256, 0, (hipStream_t)stream>>>(A);
    b0 += n;
  }
  return mi355_check_launch("patch_queue_gather_spatial");
}
