// Training patch queue (reference: src/data_module.py:125-188, TorchIO's CropOrPad -> augmentation Compose with
// keep= -> UniformSampler -> Queue): one launch writes a whole batch of patches straight from the RAW subject volumes,
//     out_j[b][ch][z][y][x] = A_b( P(src_j)[ch][o_b + (z, y, x)] )
// with the crop/pad P done by index arithmetic (the padded volume is never materialised; a pad voxel reads as the
// padding value) and the augmentation stages A_b of the patch's subject load applied in registers with the per-voxel
// math of augment_core.h, in the padded volume's coordinates, so that a patch equals
// extract_patches(chain(crop_or_pad(raw))) bit for bit.
//
// One lane owns VEC = 4 consecutive voxels of a patch row and walks every channel of its image: the bias field (a
// function of the position only) is evaluated once per lane.  Rows are contiguous along W but origins are arbitrary, so
// a source row is usually not 16-byte aligned: when the source rows are (w % 4 == 0, aligned base) a lane reads the two
// aligned 16-byte words that cover its 4 voxels and selects (the misalignment is uniform over a patch, so the select is
// a uniform branch); rows that touch the pad border take the per-voxel path.  Stores are 16 bytes per lane.
// Descriptors travel by value in the kernel arguments (~2.3 KB): no atomics, no device table, no host synchronisation.
#include "common.h"
#include "augment_core.h"

namespace {

struct QSrc { const float* src; int d, h, w, sz, sy, sx, vec; };   // raw = padded + (sz, sy, sx); vec: 16-byte rows
struct QImg { float* dst; int c, aug; };                            // dst = patch 0 of the chunk
struct QArgs {
  mi355_queue_load load[MI355_QUEUE_MAX_LOADS];
  QSrc src[MI355_QUEUE_MAX_LOADS][MI355_QUEUE_MAX_IMAGES];
  QImg img[MI355_QUEUE_MAX_IMAGES];
  int patch[MI355_MAX_PATCHES][4];                                  // local load slot, origin z, y, x (padded)
  int td, th, tw, pd, ph, pw;
  float pad;
};

constexpr int kChanUnroll = 4;   // channels whose loads are in flight together

template <int VEC>
__device__ __forceinline__ void load_run(const float* __restrict__ src, long long off, int rx, int w, bool row_in, bool fast,
                                         int m, float pad, float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    if (fast) {
      // covering aligned words: [rx - m, rx - m + 8) lies inside the row (w % 4 == 0, rx + 3 < w)
      const f32x4 a = *reinterpret_cast<const f32x4*>(src + off + rx - m);
      if (m == 0) {
        v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3];
      } else {
        const f32x4 b = *reinterpret_cast<const f32x4*>(src + off + rx - m + 4);
        if (m == 1) { v[0] = a[1]; v[1] = a[2]; v[2] = a[3]; v[3] = b[0]; }
        else if (m == 2) { v[0] = a[2]; v[1] = a[3]; v[2] = b[0]; v[3] = b[1]; }
        else { v[0] = a[3]; v[1] = b[0]; v[2] = b[1]; v[3] = b[2]; }
      }
      return;
    }
  }
#pragma unroll
  for (int k = 0; k < VEC; ++k) {
    const int xx = rx + k;
    v[k] = row_in && xx >= 0 && xx < w ? src[off + xx] : pad;
  }
}

// grid: (runs of a patch / 256, patches of the chunk, images)
template <int VEC>
__global__ __launch_bounds__(256) void patch_queue_kernel(const QArgs A) {
  const int b = blockIdx.y, j = blockIdx.z;
  const int wv = A.pw / VEC;
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= (long long)A.pd * A.ph * wv) return;
  const int z = (int)(r / ((long long)A.ph * wv)), y = (int)(r / wv % A.ph), x = (int)(r % wv) * VEC;
  const int l = A.patch[b][0];
  const int pz = A.patch[b][1] + z, py = A.patch[b][2] + y, px = A.patch[b][3] + x;   // padded coordinates
  const QSrc& S = A.src[l][j];
  const QImg& I = A.img[j];
  const mi355_queue_load& L = A.load[l];
  const int rz = pz + S.sz, ry = py + S.sy, rx = px + S.sx;                             // raw coordinates
  const bool row_in = rz >= 0 && rz < S.d && ry >= 0 && ry < S.h;
  const bool fast = VEC == 4 && S.vec && row_in && rx >= 0 && rx + VEC <= S.w;
  const int m = rx & 3;
  const long long svol = (long long)S.d * S.h * S.w;
  const long long row = row_in ? ((long long)rz * S.h + ry) * S.w : 0;
  const long long pv = (long long)A.pd * A.ph * A.pw;
  float* __restrict__ dst = I.dst + (long long)b * I.c * pv + ((long long)z * A.ph + y) * A.pw + x;
  const int ns = I.aug ? L.nstages : 0;
  const long long tvol = (long long)A.td * A.th * A.tw;
  const long long flat0 = ((long long)pz * A.th + py) * A.tw + px;                       // noise key of channel 0

  float g[VEC];                                                                           // bias field: position only
  bool bias = false;
  for (int s = 0; s < ns; ++s) bias |= L.stage[s] == MI355_STAGE_BIAS_FIELD;
  if (bias) {
#pragma unroll
    for (int k = 0; k < VEC; ++k)
      g[k] = expf(aug_bias_log_field(pz, py, px + k, A.td, A.th, A.tw, L.bias_order, L.bias_coef));
  }

  for (int c0 = 0; c0 < I.c; c0 += kChanUnroll) {
    float v[kChanUnroll][VEC];
#pragma unroll
    for (int u = 0; u < kChanUnroll; ++u)
      if (c0 + u < I.c) load_run<VEC>(S.src, (c0 + u) * svol + row, rx, S.w, row_in, fast, m, A.pad, v[u]);
#pragma unroll
    for (int u = 0; u < kChanUnroll; ++u) {
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

// raw coordinate = padded coordinate + shift: augment.crop_or_pad's centred crop ((n - t) // 2 dropped before) or pad
// ((t - n) // 2 added before)
int crop_pad_shift(int n, int t) { return n > t ? (n - t) / 2 : -((t - n) / 2); }

}  // namespace

extern "C" int mi355_patch_queue_gather(const mi355_queue_load* loads, int32_t nloads, const mi355_queue_source* sources,
                                        const int32_t* channels, const int32_t* augmented, float* const* outs, int32_t nimages,
                                        const int32_t* patches, int32_t npatches, int32_t td, int32_t th, int32_t tw,
                                        int32_t pd, int32_t ph, int32_t pw, float padding_value, void* stream) {
  MI355_REQUIRE(npatches >= 0, "patch_queue_gather: bad patch count");
  MI355_REQUIRE(td > 0 && th > 0 && tw > 0 && pd > 0 && ph > 0 && pw > 0 && pd <= td && ph <= th && pw <= tw,
                "patch_queue_gather: bad patch (%d, %d, %d) or target (%d, %d, %d) shape", pd, ph, pw, td, th, tw);
  MI355_REQUIRE(nimages > 0 && nimages <= MI355_QUEUE_MAX_IMAGES, "patch_queue_gather: 1..%d images, got %d",
                MI355_QUEUE_MAX_IMAGES, nimages);
  if (npatches == 0) return MI355_OK;
  MI355_REQUIRE(loads && sources && channels && augmented && outs && patches, "patch_queue_gather: null pointer");
  MI355_REQUIRE(nloads > 0, "patch_queue_gather: no subject load");
  for (int l = 0; l < nloads; ++l) {
    const mi355_queue_load& L = loads[l];
    MI355_REQUIRE(L.nstages >= 0 && L.nstages <= MI355_QUEUE_MAX_STAGES, "patch_queue_gather: load %d: bad stage count", l);
    int seen = 0;
    for (int s = 0; s < L.nstages; ++s) {
      const int k = L.stage[s];
      MI355_REQUIRE(k >= MI355_STAGE_BIAS_FIELD && k <= MI355_STAGE_GAMMA && !(seen & (1 << k)),
                    "patch_queue_gather: load %d: bad or repeated stage %d", l, k);
      seen |= 1 << k;
    }
    MI355_REQUIRE(L.bias_order >= 0 && L.bias_order <= 4, "patch_queue_gather: load %d: bias order must be 0..4", l);
    MI355_REQUIRE(L.noise_std >= 0.f, "patch_queue_gather: load %d: negative noise std", l);
    for (int j = 0; j < nimages; ++j) {
      const mi355_queue_source& s = sources[(long long)l * nimages + j];
      MI355_REQUIRE(s.src && s.d > 0 && s.h > 0 && s.w > 0, "patch_queue_gather: load %d image %d: bad source", l, j);
    }
  }
  bool vec = pw % 4 == 0;
  for (int j = 0; j < nimages; ++j) {
    MI355_REQUIRE(outs[j] && channels[j] > 0 && channels[j] <= 65535, "patch_queue_gather: image %d: bad output", j);
    vec = vec && ((uintptr_t)outs[j] & 15) == 0;
  }
  for (int b = 0; b < npatches; ++b) {
    const int32_t* p = patches + 4LL * b;
    MI355_REQUIRE(p[0] >= 0 && p[0] < nloads, "patch_queue_gather: patch %d: load %d out of range", b, p[0]);
    MI355_REQUIRE(p[1] >= 0 && p[1] + pd <= td && p[2] >= 0 && p[2] + ph <= th && p[3] >= 0 && p[3] + pw <= tw,
                  "patch_queue_gather: patch %d leaves the target volume", b);
  }
  const long long pv = (long long)pd * ph * pw;
  const long long runs = pv / (vec ? 4 : 1);
  for (int b0 = 0; b0 < npatches;) {
    // a chunk: at most MI355_MAX_PATCHES patches of at most MI355_QUEUE_MAX_LOADS distinct loads
    QArgs A;
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
      for (int j = 0; j < nimages; ++j) {
        const mi355_queue_source& src = sources[(long long)slot_of[s] * nimages + j];
        A.src[s][j] = QSrc{src.src, src.d, src.h, src.w, crop_pad_shift(src.d, td), crop_pad_shift(src.h, th),
                           crop_pad_shift(src.w, tw), src.w % 4 == 0 && ((uintptr_t)src.src & 15) == 0};
      }
    }
    for (int j = 0; j < nimages; ++j) A.img[j] = QImg{outs[j] + (long long)b0 * channels[j] * pv, channels[j], augmented[j] != 0};
    A.td = td; A.th = th; A.tw = tw; A.pd = pd; A.ph = ph; A.pw = pw; A.pad = padding_value;
    const dim3 grid((unsigned)((runs + 255) / 256), n, nimages);
    if (vec) patch_queue_kernel<4><<<grid, 256, 0, (hipStream_t)stream>>>(A);
    else patch_queue_kernel<1><<<grid, 256, 0, (hipStream_t)stream>>>(A);
    b0 += n;
  }
  return mi355_check_launch("patch_queue_gather");
}
