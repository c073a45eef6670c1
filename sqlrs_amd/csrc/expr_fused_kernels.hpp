// expr_fused_kernels.hpp — the two kernels of the fused-evaluation route of the synchronous Filter / Project (expr_fused.hip;
// SQLRS_EXPR_FUSED_EVAL).
//
// Both follow sr_reduce_kernel's access shape (simple_reduce_kernels.hpp): 256-thread workgroups, <= FE_MAX_BLOCKS of them,
// grid-stride; a wave owns FE_UNROLL consecutive 64-row groups per trip (lane = row inside the group: 4 or 8 B per lane,
// coalesced; the validity word of a group and the value word of a Boolean column are ONE load for the wave, at an address the
// scalar unit holds), a workgroup 4 x FE_UNROLL groups = 1024 rows, the full grid 2^21 rows.  The programs (SaProgram, compiled
// by sa_compile on the host per push) arrive as kernel arguments and are copied into LDS at kernel start; a row is one call
// of sa_eval_row (small_async.hpp: the evaluator's semantics, untouched here).
//
// fe_mask_kernel      the Filter's predicate: keep = valid && value != 0, __ballot(keep) is the selection's mask word of the
//                     group (bits past `rows`: 0), lane 0 stores it — no Boolean array, no mask conversion.
// fe_project_kernel   <= FE_MAX_PROGS computed columns per launch: the value stored at its width (0 under a NULL), a Boolean
//                     result and every validity bitmap as one ballot word per group.
// A valid row that divides by zero: lane 0 of a wave whose ballot of `div0` is non-zero stores 1 into *flag (a plain vector
// store; the host zeroes the word on the stream before the launch and passes null when no program holds a division).
#pragma once

#include "small_async.hpp"

namespace sq {

constexpr int FE_MAX_COLS = 16, FE_MAX_PROGS = 4;
constexpr int FE_THREADS = 256, FE_UNROLL = 4, FE_MAX_BLOCKS = 2048;
constexpr int FE_BLOCK_ROWS = FE_THREADS * FE_UNROLL;                      // 1024
constexpr int64_t FE_SWEEP_ROWS = (int64_t)FE_MAX_BLOCKS * FE_BLOCK_ROWS; // 2^21
enum { FE_K32 = 0, FE_K64 = 1, FE_KBOOL = 2 }; // an int32 (sign-extended into the operand word), 8 bytes, or one bit per row

// one referenced column of the batch, in the programs' numbering
struct FeCol {
  const void *values;
  const uint64_t *validity; // null: no NULLs
  uint32_t kind, pad;
};
struct FeBatch {
  FeCol c[FE_MAX_COLS];
  long long rows;
};
struct FeOut {
  void *values;       // rows x 4 / 8 bytes; FE_KBOOL: one word per group
  uint64_t *validity; // one word per group, always written
  uint32_t kind, pad;
};
template <int N> struct FePrograms {
  SaProgram p[N];
};
template <int N> struct FeOuts {
  FeOut o[N];
};

#if defined(__HIPCC__)
// operand loader of the interpreter: row r = 64 grp + lane of the batch's global columns.  `col` comes out of the program in
// LDS and is the same for the whole wave: made a scalar, so that the column's descriptor is read with scalar loads out of the
// kernel arguments and the words of the bitmaps (index grp, uniform too) with one load for the wave.
struct FeLoad {
  const FeBatch &b;
  long long r, grp;
  int lane;
  __device__ __forceinline__ unsigned long long operator()(uint32_t col, bool *ok) const {
    const FeCol &c = b.c[__builtin_amdgcn_readfirstlane((int)col)];
    const uint64_t *v = c.validity;
    *ok = !v || ((v[grp] >> lane) & 1);
    const uint32_t kind = c.kind;
    if (kind == FE_KBOOL) return (unsigned long long)((((const uint64_t *)c.values)[grp] >> lane) & 1);
    return kind == FE_K64 ? ((const unsigned long long *)c.values)[r] : (unsigned long long)(long long)((const int32_t *)c.values)[r];
  }
};

template <int N> __device__ __forceinline__ void fe_programs_to_lds(const FePrograms<N> &src, unsigned char *dst_raw) {
  const uint32_t *src32 = (const uint32_t *)&src;
  uint32_t *dst = (uint32_t *)dst_raw;
  for (uint32_t k = threadIdx.x; k < sizeof(FePrograms<N>) / 4; k += FE_THREADS) dst[k] = src32[k];
  __syncthreads();
}

__global__ void __launch_bounds__(FE_THREADS) fe_mask_kernel(FePrograms<1> progs, FeBatch b, uint64_t *__restrict__ bits, uint32_t *__restrict__ flag) {
  __shared__ __attribute__((aligned(8))) unsigned char s_raw[sizeof(FePrograms<1>)]; // (SaProgram has member initialisers)
  fe_programs_to_lds(progs, s_raw);
  const SaProgram &pr = ((const FePrograms<1> *)s_raw)->p[0];
  const long long rows = b.rows, groups = (rows + 63) >> 6;
  const int lane = lane_id(), wave = __builtin_amdgcn_readfirstlane(wave_id());
  bool div0 = false;
  for (long long g0 = ((long long)blockIdx.x * (FE_THREADS / 64) + wave) * FE_UNROLL; g0 < groups;
       g0 += (long long)gridDim.x * (FE_THREADS / 64) * FE_UNROLL) {
#pragma unroll 1
    for (int u = 0; u < FE_UNROLL; u++) {
      const long long g = g0 + u;
      if (g >= groups) break; // (uniform)
      const long long r = (g << 6) + lane;
      const bool in = r < rows;
      bool valid = false, d0 = false;
      unsigned long long m = 0;
      if (in) m = sa_eval_row<false>(pr, FeLoad{b, r, g, lane}, &valid, &d0);
      div0 |= d0;
      const uint64_t w = __ballot(in && valid && m != 0);
      if (lane == 0) bits[g] = w;
    }
  }
  const bool wave_div0 = __ballot(div0) != 0;
  if (wave_div0 && lane == 0 && flag) *flag = 1u;
}

template <int N>
__global__ void __launch_bounds__(FE_THREADS) fe_project_kernel(FePrograms<N> progs, FeBatch b, FeOuts<N> outs, uint32_t *__restrict__ flag) {
  __shared__ __attribute__((aligned(8))) unsigned char s_raw[sizeof(FePrograms<N>)];
  fe_programs_to_lds(progs, s_raw);
  const FePrograms<N> &pp = *(const FePrograms<N> *)s_raw;
  const long long rows = b.rows, groups = (rows + 63) >> 6;
  const int lane = lane_id(), wave = __builtin_amdgcn_readfirstlane(wave_id());
  bool div0 = false;
  for (long long g0 = ((long long)blockIdx.x * (FE_THREADS / 64) + wave) * FE_UNROLL; g0 < groups;
       g0 += (long long)gridDim.x * (FE_THREADS / 64) * FE_UNROLL) {
#pragma unroll 1
    for (int u = 0; u < FE_UNROLL; u++) {
      const long long g = g0 + u;
      if (g >= groups) break; // (uniform)
      const long long r = (g << 6) + lane;
      const bool in = r < rows;
#pragma unroll
      for (int p = 0; p < N; p++) { // (static index: the output descriptors stay kernel arguments)
        bool valid = false, d0 = false;
        unsigned long long m = 0;
        if (in) m = sa_eval_row<false>(pp.p[p], FeLoad{b, r, g, lane}, &valid, &d0);
        div0 |= d0;
        valid = in && valid;
        m = valid ? m : 0ull; // (the value under a NULL)
        const FeOut &o = outs.o[p];
        const uint64_t vw = __ballot(valid);
        if (o.kind == FE_KBOOL) {
          const uint64_t bw = __ballot(m != 0);
          if (lane == 0) ((uint64_t *)o.values)[g] = bw;
        } else if (o.kind == FE_K64) {
          if (in) ((unsigned long long *)o.values)[r] = m;
        } else {
          if (in) ((int32_t *)o.values)[r] = (int32_t)(uint32_t)m;
        }
        if (lane == 0) o.validity[g] = vw;
      }
    }
  }
  const bool wave_div0 = __ballot(div0) != 0;
  if (wave_div0 && lane == 0 && flag) *flag = 1u;
}
#endif

} // namespace sq
