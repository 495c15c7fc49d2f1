// MedicalNet ResNet-10 feature extractor, forward only (reference: the network inside the Perceptual term of PerceptualL1Loss,
// src/model.py:123-138, and behind the FID metric, :158-163, 235-257).  The network is frozen and runs in eval mode, so every
// BatchNorm is folded into its convolution at load time (unet_bssfp_amd/medicalnet.py): the kernels see weights and a bias.
// bf16 operands, f32 accumulation on v_mfma_f32_32x32x16_bf16; activations between layers are dense bf16 NDHWC.
//   moments : sum and sum of squares of a whole f32 tensor in f64 -> {mean, unbiased std} as two floats in DEVICE memory.
//   stem    : Conv3d(1 -> 64, k7, s2, p3) + bias + ReLU straight from the f32 NCDHW volumes (every (b, c) pair is one
//             sample).  An in-range voxel enters as bf16((x - mean) / std), a padding tap as 0 -- which is why the
//             normalisation is not folded into the weights.  The contraction is ordered (kd, kh, kw') with kw' = 0..7 (kw' = 7
//             carries a zero weight) and one zero (kd, kh) pair at the end: K = 50 * 8 = 400 = 25 MFMA steps, and one lane's
//             8-element fragment is one contiguous piece of an input row.  The weights (51 KB) sit in LDS, and so does the
//             input patch of a workgroup's 4 x 4 x 16 output tile, normalised once per voxel while it is staged.
//   pool    : MaxPool3d(k3, s2, p1) as a second kernel, 16 bytes per lane; padding counts as -inf.
//   conv    : ONE implicit-GEMM kernel for the 3x3x3 convolutions (stride 1 / 2, dilation 1 / 2 / 4, padding = dilation) and
//             the 1x1x1 downsample (ks = 1): a wave owns 64 output voxels x 64 output channels (2 x 2 MFMA tiles) and loads both
//             fragments straight from global memory, 16 bytes per lane: the activation rows are contiguous in cin, the weights
//             are packed [tap][cin / 16][cout][16].  No LDS: at 16^3 and 8^3 per sample a tap's halo is as large as the tile, and
//             the re-reads hit in L1 / L2.  Epilogue: + bias, + residual (bf16), ReLU, bf16 store.
//   tail    : one pass over the two feature tensors: per batch item the Perceptual partial sums and the spatial means for FID.
// No atomics anywhere; every reduction has a fixed order, so calls are bit-identical.  No host read: mean and std travel by
// device pointer.  What the backward (csrc/medicalnet_bwd.hip) needs as well lives in csrc/medicalnet_common.h, once: the
// implicit-GEMM loop of conv, the window scan of pool, pass 1 of tail, the tile decode of stem, the reductions and the host checks.
#include "medicalnet_common.h"

namespace {

constexpr int kStemSteps = 25;                  // MFMA steps of the stem contraction: (49 + 1) (kd, kh) pairs x 8 / 16

// ---------------------------------------------------------------------------------------------------- moments
__global__ __launch_bounds__(256) void mnet_moments_kernel(const float* __restrict__ x, long long n, double* __restrict__ part) {
  __shared__ double red[4];
  double s = 0.0, q = 0.0;
  const long long stride = (long long)gridDim.x * 256, first = (long long)blockIdx.x * 256 + threadIdx.x;
  if ((reinterpret_cast<uintptr_t>(x) & 15) == 0) {
    const long long n4 = n >> 2;
    for (long long i = first; i < n4; i += stride) {
      const float4 v = reinterpret_cast<const float4*>(x)[i];
      const double a = v.x, b = v.y, c = v.z, d = v.w;
      s += (a + b) + (c + d);
      q += (a * a + b * b) + (c * c + d * d);
    }
    for (long long i = (n4 << 2) + first; i < n; i += stride) { const double a = x[i]; s += a; q += a * a; }
  } else {
    for (long long i = first; i < n; i += stride) { const double a = x[i]; s += a; q += a * a; }
  }
  s = block_sum_256d(s, red);
  q = block_sum_256d(q, red);
  if (threadIdx.x == 0) { part[2 * blockIdx.x] = s; part[2 * blockIdx.x + 1] = q; }
}

// one workgroup: {mean, unbiased std} of the n values behind the nb partial pairs
__global__ __launch_bounds__(256) void mnet_moments_final_kernel(const double* __restrict__ part, int nb, long long n,
                                                                 float* __restrict__ out) {
  __shared__ double red[4];
  double s = 0.0, q = 0.0;
  for (int i = threadIdx.x; i < nb; i += 256) { s += part[2 * i]; q += part[2 * i + 1]; }
  s = block_sum_256d(s, red);
  q = block_sum_256d(q, red);
  if (threadIdx.x == 0) {
    const double mean = s / (double)n;
    const double var = (q - s * mean) / (double)(n - 1);
    out[0] = (float)mean;
    out[1] = (float)sqrt(var > 0.0 ? var : 0.0);
  }
}

// ---------------------------------------------------------------------------------------------------- stem
struct StemArgs {
  const float* x; const float* ms; const char* wp; const float* bias; bf16_t* y;
  int d, h, w, do_, ho, wo;
  int tiles_d, tiles_h, tiles_w;
  long long tiles;                         // samples * tiles_d * tiles_h * tiles_w
};

// Output tile of a workgroup: 4 x 4 x 16 voxels of one sample; wave = one d-slice (4 x 16 voxels = two 32-row MFMA subtiles of
// 2 x 16).  The tile's input patch, 13 x 13 x 38 voxels from (2 od0 - 3, 2 oh0 - 3, 2 ow0 - 3), is normalised ONCE per voxel while
// it is staged into LDS as bf16 (padding = 0); rows are 40 elements apart, so the 8 consecutive elements of a lane's fragment --
// input columns 2 ow - 3 .. 2 ow + 4, patch columns 2 ow_l .. 2 ow_l + 7 -- start 4-byte aligned: four ds_read_b32.
constexpr int kStemTD = 4, kStemTH = 4, kStemTW = 16;
constexpr int kPatchD = 2 * kStemTD + 5, kPatchH = 2 * kStemTH + 5, kPatchW = 2 * kStemTW + 6, kPatchPitch = 40;

__global__ __launch_bounds__(256) void mnet_stem_kernel(const StemArgs a) {
  __shared__ uint4 wlds[kStemSteps * kStemC * 2];                      // [step][cout][16] bf16, 51.2 KB
  __shared__ uint32_t patch[kPatchD * kPatchH * kPatchPitch / 2];         // bf16 pairs, 13.5 KB
  for (int i = threadIdx.x; i < kStemSteps * kStemC * 2; i += 256) wlds[i] = reinterpret_cast<const uint4*>(a.wp)[i];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  const float mean = a.ms[0], std = a.ms[1];
  const long long vol = (long long)a.d * a.h * a.w;
  float bias[2];
  bias[0] = a.bias[r]; bias[1] = a.bias[32 + r];
  uint16_t* patch16 = reinterpret_cast<uint16_t*>(patch);
  for (long long tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    const Tile t = tile_decode(tile, a.tiles_d, a.tiles_h, a.tiles_w);
    const long long s = t.s;
    const int od0 = t.td * kStemTD, oh0 = t.th * kStemTH, ow0 = t.tw * kStemTW;
    const float* src = a.x + s * vol;
    __syncthreads();                                                      // the previous tile's fragments have been read
    for (int i = threadIdx.x; i < kPatchD * kPatchH * kPatchW; i += 256) {
      const int row = i / kPatchW, j = i - row * kPatchW;
      const int pz = row / kPatchH, py = row - pz * kPatchH;
      const int id = 2 * od0 - 3 + pz, ih = 2 * oh0 - 3 + py, iw = 2 * ow0 - 3 + j;
      const bool in = (unsigned)id < (unsigned)a.d && (unsigned)ih < (unsigned)a.h && (unsigned)iw < (unsigned)a.w;
      const float v = src[in ? ((long long)id * a.h + ih) * a.w + iw : 0];   // issued at an in-bounds address either way
      patch16[row * kPatchPitch + j] = in ? f32_to_bf16_bits((v - mean) / std) : (uint16_t)0;
    }
    __syncthreads();
    f32x16 acc[2][2];
#pragma unroll
    for (int vt = 0; vt < 2; ++vt)
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[vt][ct][i] = 0.f;
    // this lane's rows: (od_l, oh_l, ow_l) = (wave, 2 vt + (r >> 4), r & 15); patch pair index of its fragment at (kd, kh) = (0, 0)
    const int base = ((2 * wave) * kPatchH + 2 * (r >> 4)) * (kPatchPitch / 2) + (r & 15);
#pragma unroll 5
    for (int kc = 0; kc < kStemSteps; ++kc) {
      const int pair = 2 * kc + h;                                        // pair 49 carries zero weights: it re-reads pair 48
      const int pc = pair < 49 ? pair : 48;
      const int kd = pc / 7, kh = pc - kd * 7;
      Frag<bf16_t> fa[2], fb[2];
#pragma unroll
      for (int vt = 0; vt < 2; ++vt) {
        const uint32_t* p = patch + base + ((kd * kPatchH) + kh + 4 * vt) * (kPatchPitch / 2);
        fa[vt].v = make_uint4(p[0], p[1], p[2], p[3]);
      }
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) fb[ct].v = wlds[(kc * kStemC + ct * 32 + r) * 2 + h];
#pragma unroll
      for (int vt = 0; vt < 2; ++vt)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) mma16(fa[vt], fb[ct], acc[vt][ct]);
    }
    const int od = od0 + wave;
#pragma unroll
    for (int vt = 0; vt < 2; ++vt)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int row = acc_row(i, h);
        const int oh = oh0 + 2 * vt + (row >> 4), ow = ow0 + (row & 15);
        if (od < a.do_ && oh < a.ho && ow < a.wo) {
          bf16_t* yp = a.y + ((((s * a.do_ + od) * a.ho + oh) * a.wo + ow) * kStemC) + r;
#pragma unroll
          for (int ct = 0; ct < 2; ++ct) Elem<bf16_t>::store(yp + ct * 32, fmaxf(acc[vt][ct][i] + bias[ct], 0.f));
        }
      }
  }
}

// ---------------------------------------------------------------------------------------------------- max-pool k3 s2 p1
// one thread per (output voxel, 8 channels); rows of c channels, c % 8 == 0
__global__ __launch_bounds__(256) void mnet_maxpool_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ y, long long total,
                                                           int d, int h, int w, int od_, int oh_, int ow_, int c) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  pool_scan<false>(x, i, d, h, w, od_, oh_, ow_, c, [=](long long out, const float (&best)[8]) {
    Vec16<bf16_t> o;
#pragma unroll
    for (int k = 0; k < 8; ++k) o.f[k] = best[k];
    o.store(y + out);
  });
}

// ---------------------------------------------------------------------------------------------------- residual convolutions
struct MnetConvArgs {
  const bf16_t* x; const bf16_t* wp; const float* bias; const bf16_t* res; bf16_t* y;
  int di, hi, wi, do_, ho, wo;
  int cin, cout, ks, stride, dil, pad, relu;
  long long m_total;                       // samples * do * ho * wo
};

// grid (ceil(m_total / 256), cout / 64); wave = 64 voxels x 64 channels
__global__ __launch_bounds__(256) void mnet_conv_kernel(const MnetConvArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  const long long m0 = ((long long)blockIdx.x * 4 + wave) * 64;
  if (m0 >= a.m_total) return;                                // wave-uniform; the kernel has no barrier
  const int co_base = blockIdx.y * 64;
  const long long per = (long long)a.do_ * a.ho * a.wo;
  long long sbase[2]; int id0[2], ih0[2], iw0[2]; bool ok[2];
#pragma unroll
  for (int vt = 0; vt < 2; ++vt) {
    const long long m = m0 + vt * 32 + r;
    ok[vt] = m < a.m_total;
    const long long mm = ok[vt] ? m : 0;
    const long long s = mm / per; const int rem = (int)(mm - s * per);
    const int od = rem / (a.ho * a.wo), r2 = rem - od * (a.ho * a.wo);
    const int oh = r2 / a.wo, ow = r2 - oh * a.wo;
    sbase[vt] = s * a.di;
    id0[vt] = od * a.stride - a.pad; ih0[vt] = oh * a.stride - a.pad; iw0[vt] = ow * a.stride - a.pad;
  }
  // the source voxel of row 32 vt + r at tap (kd, kh, kw): input voxel (od, oh, ow) stride - pad + tap dil
  const auto gather = [=](int vt, int kd, int kh, int kw, const bf16_t*& p) {
    const int id = id0[vt] + kd * a.dil, ih = ih0[vt] + kh * a.dil, iw = iw0[vt] + kw * a.dil;
    const bool in = ok[vt] && (unsigned)id < (unsigned)a.di && (unsigned)ih < (unsigned)a.hi && (unsigned)iw < (unsigned)a.wi;
    const long long vox = in ? ((sbase[vt] + id) * a.hi + ih) * a.wi + iw : 0;       // padding reads voxel 0: in-bounds
    p = a.x + vox * a.cin;
    return in;
  };
  const auto epilogue = [=](const f32x16 (&acc)[2][2]) {
    float bias[2];
    bias[0] = a.bias[co_base + r]; bias[1] = a.bias[co_base + 32 + r];
#pragma unroll
    for (int vt = 0; vt < 2; ++vt)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const long long m = m0 + vt * 32 + acc_row(i, h);
        if (m < a.m_total) {
#pragma unroll
          for (int ct = 0; ct < 2; ++ct) {
            const long long off = m * a.cout + co_base + ct * 32 + r;
            float v = acc[vt][ct][i] + bias[ct];
            if (a.res) v += Elem<bf16_t>::load(a.res + off);
            if (a.relu) v = fmaxf(v, 0.f);
            Elem<bf16_t>::store(a.y + off, v);
          }
        }
      }
  };
  gemm_wave(a.wp, a.ks, a.cin >> 4, a.cout, co_base, r, h, gather, epilogue);   // wp: [tap][cin / 16][cout][16]
}

// ---------------------------------------------------------------------------------------------------- tail
// grid (chunks, items): item b, voxels [chunk * 16, + 16).  fp / ft: [items * c][vox][512] bf16.  A voxel's feature vector is
// the c * 512 channels of its c samples.  Writes the chunk's channel sums of both tensors and its Perceptual partial sum.
__global__ __launch_bounds__(256) void mnet_tail_kernel(const bf16_t* __restrict__ fp, const bf16_t* __restrict__ ft, int c,
                                                        int vox, float* __restrict__ colp, float* __restrict__ colt,
                                                        double* __restrict__ part) {
  __shared__ float red[4][2 * kTailVox];
  __shared__ float norm[2 * kTailVox];
  __shared__ double dred[4];
  const int b = blockIdx.y, chunk = blockIdx.x, v0 = chunk * kTailVox;
  const int nvec = c * (kFeat / 8);                                       // 16-byte vectors per voxel
  tail_sums<2>(fp, ft, b, c, vox, v0, red);                               // pass 1: p . p and t . t per voxel
  if (threadIdx.x < 2 * kTailVox) {
    const int i = threadIdx.x;
    norm[i] = sqrtf((red[0][i] + red[1][i]) + (red[2][i] + red[3][i])) + 1e-10f;
  }
  __syncthreads();
  // pass 2: channel sums over the chunk's voxels, and sum (p / |p| - t / |t|)^2
  float acc = 0.f;
  for (int ev = threadIdx.x; ev < nvec; ev += 256) {
    const long long base = tail_base(b, c, ev, vox);
    Vec16<bf16_t> sp, st;
#pragma unroll
    for (int k = 0; k < 8; ++k) { sp.f[k] = 0.f; st.f[k] = 0.f; }
#pragma unroll
    for (int vi = 0; vi < kTailVox; ++vi) {
      if (v0 + vi < vox) {
        Vec16<bf16_t> p, t;
        p.load(fp + base + (long long)(v0 + vi) * kFeat);
        t.load(ft + base + (long long)(v0 + vi) * kFeat);
        const float np = norm[2 * vi], nt = norm[2 * vi + 1];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          sp.f[k] += p.f[k]; st.f[k] += t.f[k];
          const float dlt = p.f[k] / np - t.f[k] / nt;
          acc += dlt * dlt;
        }
      }
    }
    const long long o = ((long long)b * gridDim.x + chunk) * nvec * 8 + (long long)ev * 8;
    *reinterpret_cast<float4*>(colp + o) = make_float4(sp.f[0], sp.f[1], sp.f[2], sp.f[3]);
    *reinterpret_cast<float4*>(colp + o + 4) = make_float4(sp.f[4], sp.f[5], sp.f[6], sp.f[7]);
    *reinterpret_cast<float4*>(colt + o) = make_float4(st.f[0], st.f[1], st.f[2], st.f[3]);
    *reinterpret_cast<float4*>(colt + o + 4) = make_float4(st.f[4], st.f[5], st.f[6], st.f[7]);
  }
  const double t = block_sum_256d((double)acc, dred);
  if (threadIdx.x == 0) part[(long long)b * gridDim.x + chunk] = t;
}

// grid (ceil(c * 512 / 256), items): spatial means of both tensors; thread 0 of the first workgroup of an item sums the item's
// Perceptual partials, and workgroup (0, 0) the value over all items (chunk by chunk, item by item: a fixed order)
__global__ __launch_bounds__(256) void mnet_tail_final_kernel(const float* __restrict__ colp, const float* __restrict__ colt,
                                                              const double* __restrict__ part, int chunks, int items, int ch,
                                                              int vox, float* __restrict__ meanp, float* __restrict__ meant,
                                                              float* __restrict__ item_sum, float* __restrict__ value) {
  const int b = blockIdx.y, e = blockIdx.x * 256 + threadIdx.x;
  if (e < ch) {
    float sp = 0.f, st = 0.f;
    for (int k = 0; k < chunks; ++k) {
      const long long o = ((long long)b * chunks + k) * ch + e;
      sp += colp[o]; st += colt[o];
    }
    meanp[(long long)b * ch + e] = sp / (float)vox;
    meant[(long long)b * ch + e] = st / (float)vox;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    double s = 0.0;
    for (int k = 0; k < chunks; ++k) s += part[(long long)b * chunks + k];
    item_sum[b] = (float)s;
    if (b == 0) {
      double tot = 0.0;
      for (int i = 0; i < items; ++i) {
        double si = 0.0;
        for (int k = 0; k < chunks; ++k) si += part[(long long)i * chunks + k];
        tot += si;
      }
      value[0] = (float)(tot / ((double)items * vox));
    }
  }
}

int moments_blocks(long long n) {
  const long long b = (n + 256 * 32 - 1) / (256 * 32);
  return (int)(b < 1 ? 1 : (b > 1024 ? 1024 : b));
}

}  // namespace

extern "C" int32_t mi355_medicalnet_moments_blocks(int64_t n) { return n > 0 ? moments_blocks(n) : 0; }

extern "C" int mi355_medicalnet_moments(const float* x, int64_t n, double* part, float* mean_std, void* stream) {
  MI355_REQUIRE(x && part && mean_std, "medicalnet_moments: null pointer");
  MI355_REQUIRE(n >= 2, "medicalnet_moments: the unbiased std needs at least two values (n=%lld)", (long long)n);
  hipStream_t st = (hipStream_t)stream;
  const int nb = moments_blocks(n);
  mnet_moments_kernel<<<nb, 256, 0, st>>>(x, n, part);
  mnet_moments_final_kernel<<<1, 256, 0, st>>>(part, nb, n, mean_std);
  return mi355_check_launch("medicalnet_moments");
}

extern "C" int mi355_medicalnet_stem(const float* x, const float* mean_std, const void* wp, const float* bias, void* y,
                                     int32_t samples, int32_t d, int32_t h, int32_t w, void* stream) {
  MI355_REQUIRE(x && mean_std && wp && bias && y, "medicalnet_stem: null pointer");
  MI355_REQUIRE(samples > 0 && d > 0 && h > 0 && w > 0, "medicalnet_stem: bad shape (samples=%d d=%d h=%d w=%d)", samples, d, h, w);
  MI355_REQUIRE((reinterpret_cast<uintptr_t>(wp) & 15) == 0, "medicalnet_stem: packed weights must be 16-byte aligned");
  StemArgs a;
  a.x = x; a.ms = mean_std; a.wp = (const char*)wp; a.bias = bias; a.y = (bf16_t*)y;
  a.d = d; a.h = h; a.w = w;
  a.do_ = out_extent(d, 7, 2, 1); a.ho = out_extent(h, 7, 2, 1); a.wo = out_extent(w, 7, 2, 1);
  MNET_SUPPORTED((long long)d * h * w < (1ll << 31) && (long long)samples * a.do_ * a.ho * a.wo < (1ll << 40),
                 "medicalnet_stem: volume too large (d=%d h=%d w=%d)", d, h, w);
  a.tiles_d = ceil_div(a.do_, kStemTD); a.tiles_h = ceil_div(a.ho, kStemTH); a.tiles_w = ceil_div(a.wo, kStemTW);
  a.tiles = (long long)samples * a.tiles_d * a.tiles_h * a.tiles_w;
  const int grid = (int)(a.tiles < 1024 ? a.tiles : 1024);    // the 51.2 KB weight copy is amortised over the tiles a workgroup walks
  mnet_stem_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(a);
  return mi355_check_launch("medicalnet_stem");
}

extern "C" int mi355_medicalnet_maxpool(const void* x, void* y, int32_t samples, int32_t d, int32_t h, int32_t w, int32_t c,
                                        void* stream) {
  MI355_REQUIRE(x && y, "medicalnet_maxpool: null pointer");
  MI355_REQUIRE(samples > 0 && d > 0 && h > 0 && w > 0 && c > 0 && c % 8 == 0,
                "medicalnet_maxpool: bad shape (samples=%d d=%d h=%d w=%d c=%d)", samples, d, h, w, c);
  const int od = out_extent(d, 3, 2, 1), oh = out_extent(h, 3, 2, 1), ow = out_extent(w, 3, 2, 1);
  const long long total = (long long)samples * od * oh * ow * (c / 8);
  MNET_SUPPORTED(total < (1ll << 39), "medicalnet_maxpool: tensor too large for one launch");
  mnet_maxpool_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>((const bf16_t*)x, (bf16_t*)y, total, d, h, w,
                                                                                       od, oh, ow, c);
  return mi355_check_launch("medicalnet_maxpool");
}

extern "C" int mi355_medicalnet_conv(const void* x, const void* wp, const float* bias, const void* residual, void* y,
                                     int32_t samples, int32_t d, int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t ks,
                                     int32_t stride, int32_t dilation, int32_t relu, void* stream) {
  MI355_REQUIRE(x && wp && bias && y, "medicalnet_conv: null pointer");
  const int rc = check_conv_args("medicalnet_conv", "x", x, wp, samples, d, h, w, cin, cout, ks, stride, dilation);
  if (rc != MI355_OK) return rc;
  MnetConvArgs a;
  a.x = (const bf16_t*)x; a.wp = (const bf16_t*)wp; a.bias = bias; a.res = (const bf16_t*)residual; a.y = (bf16_t*)y;
  a.di = d; a.hi = h; a.wi = w;
  a.do_ = out_extent(d, ks, stride, dilation); a.ho = out_extent(h, ks, stride, dilation); a.wo = out_extent(w, ks, stride, dilation);
  a.cin = cin; a.cout = cout; a.ks = ks; a.stride = stride; a.dil = dilation; a.pad = dilation * (ks / 2); a.relu = relu;
  a.m_total = (long long)samples * a.do_ * a.ho * a.wo;
  MNET_SUPPORTED((long long)a.do_ * a.ho * a.wo < (1ll << 31) && a.m_total < (1ll << 38),
                 "medicalnet_conv: tensor too large for one launch");
  mnet_conv_kernel<<<dim3((unsigned)ceil_div(a.m_total, 256), cout / 64), 256, 0, (hipStream_t)stream>>>(a);
  return mi355_check_launch("medicalnet_conv");
}

extern "C" int64_t mi355_medicalnet_tail_workspace_bytes(int32_t items, int32_t c, int32_t vox) {
  if (items <= 0 || c <= 0 || vox <= 0) return -1;
  const long long chunks = (vox + kTailVox - 1) / kTailVox;
  return 2 * (long long)items * chunks * c * kFeat * 4 + (long long)items * chunks * 8 + 256;
}

extern "C" int mi355_medicalnet_tail(const void* feat_pred, const void* feat_target, int32_t items, int32_t c, int32_t vox,
                                     void* workspace, int64_t workspace_bytes, float* mean_pred, float* mean_target,
                                     float* item_sum, float* value, void* stream) {
  const long long need = mi355_medicalnet_tail_workspace_bytes(items, c, vox);
  MI355_REQUIRE(need > 0, "medicalnet_tail: bad shape (items=%d c=%d vox=%d)", items, c, vox);
  MI355_REQUIRE(feat_pred && feat_target && workspace && mean_pred && mean_target && item_sum && value && workspace_bytes >= need,
                "medicalnet_tail: null pointer or workspace too small");
  MI355_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "medicalnet_tail: workspace must be 16-byte aligned");
  MNET_SUPPORTED(items <= 65535 && c <= 4096, "medicalnet_tail: at most 65535 items of at most 4096 channels");
  const int chunks = (vox + kTailVox - 1) / kTailVox, ch = c * kFeat;
  float* colp = (float*)workspace;
  float* colt = colp + (long long)items * chunks * ch;
  double* part = (double*)(((uintptr_t)(colt + (long long)items * chunks * ch) + 255) & ~(uintptr_t)255);
  hipStream_t st = (hipStream_t)stream;
  mnet_tail_kernel<<<dim3(chunks, items), 256, 0, st>>>((const bf16_t*)feat_pred, (const bf16_t*)feat_target, c, vox, colp, colt, part);
  mnet_tail_final_kernel<<<dim3((ch + 255) / 256, items), 256, 0, st>>>(colp, colt, part, chunks, items, ch, vox, mean_pred,
                                                                        mean_target, item_sum, value);
  return mi355_check_launch("medicalnet_tail");
}
