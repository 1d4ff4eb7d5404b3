// One wave's share of a 128 x 128 tile of C = A B in f32 MFMA (k_grm of gnx_grm.hip, k_quad of
// gnx_quad.hip).  The 2 x 2 waves of a 256-thread block each own 64 x 64 of the tile as 2 x 2
// accumulators of v_mfma_f32_32x32x2_f32.  A stage is MM_KS steps of the reduction in LDS,
// A as [k][row] and B as [k][column]; lane l takes A[i = l & 31][k = l >> 5] and
// B[k = l >> 5][j = l & 31], one float each, so lanes 0..31 read consecutive floats of step 2 kk
// and lanes 32..63 of step 2 kk + 1.  How a stage is filled, what is prefetched under the MFMAs
// and what becomes of the sums is the kernel's own.
//
// Numerics.  The MFMA result is a k-ordered fp32 fma chain.  The kernel calls flush() after at
// most 1024 products (its own constant): the fp32 accumulators are added into fp64 registers and
// cleared, so no fp32 chain is longer than that, and the fp64 sum runs in the order of the
// reduction.  No atomics: a repeated call is bit-equal.  What contributes nothing expands to
// 0.0f, never to val[l][0] (non-zero for a centred locus): geno_tables (gnx_geno.h) zeroes the
// loci outside the mask and the padding bits, and an individual past n reads entry 3, which is 0.
#pragma once
#include <cstdint>

#define MM_T 128         // tile edge
#define MM_KS 32         // steps of the reduction per LDS stage

typedef float f32x16 __attribute__((ext_vector_type(16)));

// the lane's operand in a stage S [MM_KS][MM_T] for the wave's 64 rows or columns from `first`
__device__ __forceinline__ const float* mm_operand(const float (*S)[MM_T], int first, int lane) {
  return &S[lane >> 5][first + (lane & 31)];
}

// C/D of the 32 x 32 MFMA: column = lane & 31, and the row of the lane's element e, counted
// from the accumulator's first row (added term by term: the constants fold into `first`)
__device__ __forceinline__ int64_t mm_row(int64_t first, int e, int lane) {
  return first + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
}

// the value of locus l of a word's table t [bit][4] for the dosage of bit l of a and b; dead = 3
// selects entry 3 (0) whatever the bits
__device__ __forceinline__ float mm_dosage(const float* t, unsigned a, unsigned b, int l,
                                           unsigned dead) {
  return t[l * 4 + ((((a >> l) & 1u) + ((b >> l) & 1u)) | dead)];
}

struct MmWave {
  f32x16 acc[2][2];
  double sum[2][2][16];

  __device__ __forceinline__ void clear() {
    acc[0][0] = acc[0][1] = acc[1][0] = acc[1][1] = 0.f;
#pragma unroll
    for (int q = 0; q < 64; ++q) (&sum[0][0][0])[q] = 0.0;
  }

  // one stage: sa, sb = mm_operand of the A and B stages
  __device__ __forceinline__ void stage(const float* sa, const float* sb) {
#pragma unroll 4
    for (int kk = 0; kk < MM_KS / 2; ++kk) {
      const float a0 = sa[(2 * kk) * MM_T], a1 = sa[(2 * kk) * MM_T + 32];
      const float b0 = sb[(2 * kk) * MM_T], b1 = sb[(2 * kk) * MM_T + 32];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
  }

  // the fp32 chains into the fp64 sums, in index order
  __device__ __forceinline__ void flush() {
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          sum[m][c][e] += (double)acc[m][c][e];
          acc[m][c][e] = 0.f;
        }
  }
};
