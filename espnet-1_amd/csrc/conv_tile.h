// The LDS chunk, its 8-element loads / stores and the per-chunk MFMA loop shared by the implicit-GEMM
// convolutions (vgg2l.hip, conv_sub.hip): f32 on v_mfma_f32_16x16x4_f32, bf16 on
// v_mfma_f32_16x16x32_bf16, f32 accumulation.
#pragma once
#include "common.h"

namespace {

constexpr int KC = 32;  // K elements per LDS chunk (channels of one tap / pixels of the wgrad)

template <typename T> struct Lds;
template <> struct Lds<float> { static constexpr int LD = KC + 4; };
template <> struct Lds<bf16> { static constexpr int LD = KC + 8; };

template <typename T>
EA_DEV void plain_load8(const T* p, float (&v)[8]) {
  float a[4], b[4];
  vld4(p, a);
  vld4(p + 4, b);
#pragma unroll
  for (int e = 0; e < 4; ++e) { v[e] = a[e]; v[4 + e] = b[e]; }
}

template <typename T>
EA_DEV void lds_store8(T* p, const float (&v)[8]) {
  const float a[4] = {v[0], v[1], v[2], v[3]}, b[4] = {v[4], v[5], v[6], v[7]};
  vst4(p, a);
  vst4(p + 4, b);
}

// one chunk's MFMAs of a wave: rows arow (NI tiles of 16) of As against NJ column tiles of Bs
template <typename T, int NI, int NJ>
EA_DEV void chunk_mma(const T* As, const T* Bs, int arow, int lane, f32x4 (&acc)[NI][NJ]) {
  constexpr int LD = Lds<T>::LD;
  const int r = lane & 15, q = lane >> 4;
  if constexpr (sizeof(T) == 2) {
    bf16x8 fa[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) fa[i] = *(const bf16x8*)(As + (arow + i * 16 + r) * LD + 8 * q);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const bf16x8 fb = *(const bf16x8*)(Bs + (j * 16 + r) * LD + 8 * q);
#pragma unroll
      for (int i = 0; i < NI; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb, acc[i][j], 0, 0, 0);
    }
  } else {
#pragma unroll
    for (int ks = 0; ks < KC / 4; ++ks) {
      float fa[NI];
#pragma unroll
      for (int i = 0; i < NI; ++i) fa[i] = As[(arow + i * 16 + r) * LD + ks * 4 + q];
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const float fb = Bs[(j * 16 + r) * LD + ks * 4 + q];
#pragma unroll
        for (int i = 0; i < NI; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i], fb, acc[i][j], 0, 0, 0);
      }
    }
  }
}

}  // namespace
