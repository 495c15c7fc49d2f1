// Trilinear resampling through an index-space matrix (sitk.Resample with a linear interpolator, voxel spacing 1, physical
// point = voxel index), shared by motion.hip (whole volumes) and spatial.hip (the patch gather).  Output voxel i reads the
// input at s = M i, three fmas per axis in f32 from the integer index.  Inside iff -0.5 <= s_a < N_a - 0.5 on every axis;
// then trilinear between floor(s) and floor(s) + 1, both clamped into [0, N_a - 1].  Every operation that rounds is
// written out (fmaf, one subtraction per weight, lerp), so the two users compute the same bits.
#pragma once

#include <hip/hip_runtime.h>

// s_a = m[4 a] i_D + m[4 a + 1] i_H + m[4 a + 2] i_W + m[4 a + 3]: the first three rows of the index-space matrix
struct Rigid { float m[12]; };

__device__ __forceinline__ float lerp(float a, float b, float t) { return fmaf(t, b - a, a); }

// where one output voxel reads: the inside test, the clamped corners and the weights along the three axes
struct ResamplePoint {
  bool inside;
  int lo0, hi0, lo1, hi1, lo2, hi2;
  float t0, t1, t2;
};

__device__ __forceinline__ ResamplePoint resample_point(const Rigid& q, int d, int h, int w, int id, int ih, int iw) {
  ResamplePoint p;
  const float fd = (float)id, fh = (float)ih, fw = (float)iw;
  const float s0 = fmaf(q.m[2], fw, fmaf(q.m[1], fh, fmaf(q.m[0], fd, q.m[3])));
  const float s1 = fmaf(q.m[6], fw, fmaf(q.m[5], fh, fmaf(q.m[4], fd, q.m[7])));
  const float s2 = fmaf(q.m[10], fw, fmaf(q.m[9], fh, fmaf(q.m[8], fd, q.m[11])));
  p.inside = s0 >= -0.5f && s0 < (float)d - 0.5f && s1 >= -0.5f && s1 < (float)h - 0.5f && s2 >= -0.5f &&
             s2 < (float)w - 0.5f;
  const float f0 = floorf(s0), f1 = floorf(s1), f2 = floorf(s2);
  p.t0 = s0 - f0; p.t1 = s1 - f1; p.t2 = s2 - f2;
  const int a0 = (int)f0, a1 = (int)f1, a2 = (int)f2;                 // -1 .. N - 1 when inside
  p.lo0 = max(a0, 0); p.hi0 = min(a0 + 1, d - 1);
  p.lo1 = max(a1, 0); p.hi1 = min(a1 + 1, h - 1);
  p.lo2 = max(a2, 0); p.hi2 = min(a2 + 1, w - 1);
  return p;
}

// the eight corner values v[corner along D][corner along H][corner along W] -> the interpolated value
__device__ __forceinline__ float trilinear(const float (&v)[2][2][2], float t0, float t1, float t2) {
  const float v00 = lerp(v[0][0][0], v[0][0][1], t2), v01 = lerp(v[0][1][0], v[0][1][1], t2);
  const float v10 = lerp(v[1][0][0], v[1][0][1], t2), v11 = lerp(v[1][1][0], v[1][1][1], t2);
  return lerp(lerp(v00, v01, t1), lerp(v10, v11, t1), t0);
}

// one output voxel (id, ih, iw) of one channel `xc` of a whole (d, h, w) volume: coordinate, test and gather in one piece
__device__ __forceinline__ float sample(const float* __restrict__ xc, const Rigid& q, int d, int h, int w, int id, int ih,
                                        int iw, float fill) {
  const float fd = (float)id, fh = (float)ih, fw = (float)iw;
  const float s0 = fmaf(q.m[2], fw, fmaf(q.m[1], fh, fmaf(q.m[0], fd, q.m[3])));
  const float s1 = fmaf(q.m[6], fw, fmaf(q.m[5], fh, fmaf(q.m[4], fd, q.m[7])));
  const float s2 = fmaf(q.m[10], fw, fmaf(q.m[9], fh, fmaf(q.m[8], fd, q.m[11])));
  const bool inside = s0 >= -0.5f && s0 < (float)d - 0.5f && s1 >= -0.5f && s1 < (float)h - 0.5f && s2 >= -0.5f &&
                      s2 < (float)w - 0.5f;
  if (!inside) return fill;
  const float f0 = floorf(s0), f1 = floorf(s1), f2 = floorf(s2);
  const float t0 = s0 - f0, t1 = s1 - f1, t2 = s2 - f2;
  const int a0 = (int)f0, a1 = (int)f1, a2 = (int)f2;                 // -1 .. N - 1
  const int lo0 = max(a0, 0), hi0 = min(a0 + 1, d - 1);
  const int lo1 = max(a1, 0), hi1 = min(a1 + 1, h - 1);
  const int lo2 = max(a2, 0), hi2 = min(a2 + 1, w - 1);
  const float* __restrict__ p00 = xc + ((long long)lo0 * h + lo1) * w;
  const float* __restrict__ p01 = xc + ((long long)lo0 * h + hi1) * w;
  const float* __restrict__ p10 = xc + ((long long)hi0 * h + lo1) * w;
  const float* __restrict__ p11 = xc + ((long long)hi0 * h + hi1) * w;
  const float v00 = lerp(p00[lo2], p00[hi2], t2), v01 = lerp(p01[lo2], p01[hi2], t2);
  const float v10 = lerp(p10[lo2], p10[hi2], t2), v11 = lerp(p11[lo2], p11[hi2], t2);
  return lerp(lerp(v00, v01, t1), lerp(v10, v11, t1), t0);
}
