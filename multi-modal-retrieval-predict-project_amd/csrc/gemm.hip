#include <algorithm>
// bf16 "linear" GEMM with fused epilogue for the towers (gfx950):
//   Y[m][n] = act(sum_k X[m][k] * W[n][k] + bias[n]) (+ R[m][n]),  X, W, R, Y bf16, f32 accumulate.
// nn.Linear layout (W = [out][in]): both operands K-contiguous, so both MFMA fragments are 16-byte
// row reads.  Replaces every nn.Linear of timm Swin / HF BERT on the path (fusion.py:198-199,
// 322-325): QKV, attention output (+residual), FFN1 (+GELU), FFN2 (+residual), PatchMerging
// reduction, and the 4x4/s4 patch-embed conv as an im2col GEMM.
//
// Structure (cdna_hip_programming.md §5 "minimum 2-phase" + glds + T1/T2):
//  * tile 128x128x64, 256 threads = 4 waves (2x2), wave tile 64x64 = 4x4 v_mfma_f32_16x16x32_bf16;
//  * operands go HBM -> LDS with global_load_lds_dwordx4 (no VGPR staging); the LDS image is
//    lane-linear per wave instruction (8 rows x 128 B), and the bank-conflict swizzle
//    (16-B chunk c of row r lives at chunk c ^ ((r>>1)&7)) is applied on the per-lane SOURCE
//    address and again on the ds_read_b128 fragment read (rule 21: same involution both sides);
//  * rows past M / N and chunks past K read a 16-byte zero page, so tails need no branches;
//  * two LDS stages: the loads of k-tile t+1 are issued before the MFMAs of tile t;
//  * XCD-aware bijective block remap: the N/128 tiles sharing one 128-row X panel run on one XCD;
//  * epilogue: bias + GELU in registers, tile staged through LDS as bf16, then written (with the
//    residual add) as 16-byte row chunks — coalesced 128-B rows instead of 2-byte scatters.
#include <stdlib.h>

#include <map>
#include <mutex>
#include <utility>

#include <stdio.h>

#include "common.h"

namespace {

using mmr::aligned16;
using mmr::bf16x8;
using mmr::cu_count;
using mmr::f16x8;
using mmr::f32x4;
using mmr::LGKM0;
using mmr::u32x2;
using mmr::u32x4;
using mmr::vmcnt_n;
typedef int i32x4_t __attribute__((ext_vector_type(4)));

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int TILE = BM * BK;          // bf16 elements per operand per stage (16 KiB)
constexpr int EPI_LD = 64 + 8;         // bf16 row stride of a wave's 64x64 epilogue tile
constexpr size_t EPI_BIG_B = 8 * 64 * EPI_LD * 2;  // epilogue staging of the 8-wave kernels

__device__ __attribute__((aligned(16))) uint4 g_zero_page[4];  // zero-initialised

__device__ __forceinline__ int swz(int row, int chunk) { return chunk ^ ((row >> 1) & 7); }

typedef __attribute__((address_space(3))) void* lds_ptr_t;

template <int ACT, bool HAS_BIAS, bool HAS_RES>
__global__ __launch_bounds__(256, 2) void gemm_bf16_tn(const uint16_t* __restrict__ X,
                                                        const uint16_t* __restrict__ W,
                                                        const float* __restrict__ bias,
                                                        const uint16_t* __restrict__ R,
                                                        uint16_t* __restrict__ Y, int64_t M, int N,
                                                        int K, int tiles_m, int tiles_n) {
  __shared__ __attribute__((aligned(16))) uint16_t lds[2 * 2 * TILE];  // [stage][A|B][128][64]

  const int nwg = tiles_m * tiles_n;
  const int orig = blockIdx.x;
  const int q = nwg / 8, r8 = nwg % 8, xcd = orig % 8;
  const int wg = (xcd < r8 ? xcd * (q + 1) : r8 * (q + 1) + (xcd - r8) * q) + orig / 8;
  const int tm = wg / tiles_n, tn = wg % tiles_n;
  const int64_t m0 = (int64_t)tm * BM;
  const int n0 = tn * BN;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;

  // glds addressing: wave w stages rows [32w, 32w+32) of each operand, 4 instructions of 8 rows;
  // lane i of instruction j writes LDS row 32w + 8j + i/8, physical chunk i%8.
  const int prow_in = lane >> 3, pch = lane & 7;
  const uint16_t* srcA[4];
  const uint16_t* srcB[4];
  int lchk[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int row = wave * 32 + j * 8 + prow_in;
    lchk[j] = swz(row, pch) * 8;  // logical k offset (elements) this lane fetches within a k-tile
    const int64_t gm = m0 + row;
    const int gn = n0 + row;
    srcA[j] = gm < M ? X + gm * K : nullptr;
    srcB[j] = gn < N ? W + (int64_t)gn * K : nullptr;
  }
  const uint16_t* zp = (const uint16_t*)g_zero_page;

  auto stage = [&](int s, int k0) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = k0 + lchk[j];
      const bool kin = k < K;
      const uint16_t* a = (srcA[j] && kin) ? srcA[j] + k : zp;
      const uint16_t* b = (srcB[j] && kin) ? srcB[j] + k : zp;
      uint16_t* la = lds + (s * 2 + 0) * TILE + (wave * 32 + j * 8) * BK;
      uint16_t* lb = lds + (s * 2 + 1) * TILE + (wave * 32 + j * 8) * BK;
      __builtin_amdgcn_global_load_lds((const void*)a, (lds_ptr_t)la, 16, 0, 0);
      __builtin_amdgcn_global_load_lds((const void*)b, (lds_ptr_t)lb, 16, 0, 0);
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int nk = (K + BK - 1) / BK;
  const int fr = lane & 15, fq = lane >> 4;
  stage(0, 0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int s = kt & 1;
    if (kt + 1 < nk) stage(s ^ 1, (kt + 1) * BK);
    const uint16_t* la = lds + (s * 2 + 0) * TILE;
    const uint16_t* lb = lds + (s * 2 + 1) * TILE;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 a[4], b[4];
      const int ch = ks * 4 + fq;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int rowa = wm * 64 + i * 16 + fr;
        const int rowb = wn * 64 + i * 16 + fr;
        a[i] = *(const bf16x8*)(la + rowa * BK + swz(rowa, ch) * 8);
        b[i] = *(const bf16x8*)(lb + rowb * BK + swz(rowb, ch) * 8);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[j], a[i], acc[i][j], 0, 0, 0);
    }
    __syncthreads();  // waits the in-flight glds (vmcnt(0)) and every wave's reads of stage s
  }

  // ---- epilogue: bias/act in registers -> bf16 tile in LDS -> 16-B row chunks (+ residual).
  // acc holds C^T tiles (operands swapped): lane l has row m = 16i + (l&15) and the 4
  // consecutive columns n = 16j + 4(l>>4) + 0..3, written to LDS as one 8-byte store.
  uint16_t* et = lds + wave * 64 * EPI_LD;  // reuses the (now idle) staging buffers
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int nl = j * 16 + fq * 4;
    const int n = n0 + wn * 64 + nl;
    float4 bv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (HAS_BIAS && n < N) bv = *(const float4*)(bias + n);
    const float bb[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float v[4];
#pragma unroll
      for (int rg = 0; rg < 4; ++rg) {
        v[rg] = acc[i][j][rg] + bb[rg];
        if (ACT == 1) v[rg] = mmr::gelu_fast(v[rg]);
      }
      uint2 pk;
      pk.x = mmr::pack2bf(v[0], v[1]);
      pk.y = mmr::pack2bf(v[2], v[3]);
      *(uint2*)(et + (i * 16 + fr) * EPI_LD + nl) = pk;
    }
  }
  __builtin_amdgcn_s_waitcnt(LGKM0);  // lgkmcnt(0): this wave's LDS writes landed
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int it = 0; it < 8; ++it) {
    const int c = it * 64 + lane;
    const int rl = c >> 3, cc = (c & 7) * 8;
    const int64_t m = m0 + wm * 64 + rl;
    const int n = n0 + wn * 64 + cc;
    if (m >= M || n >= N) continue;
    bf16x8 v = *(const bf16x8*)(et + rl * EPI_LD + cc);
    if (HAS_RES) {
      const bf16x8 rr = *(const bf16x8*)(R + m * N + n);
      uint32_t o[4];
#pragma unroll
      for (int e = 0; e < 4; ++e)
        o[e] = mmr::pack2bf(mmr::bf2f((uint16_t)v[2 * e]) + mmr::bf2f((uint16_t)rr[2 * e]),
                            mmr::bf2f((uint16_t)v[2 * e + 1]) + mmr::bf2f((uint16_t)rr[2 * e + 1]));
      v = __builtin_bit_cast(bf16x8, make_uint4(o[0], o[1], o[2], o[3]));
    }
    *(bf16x8*)(Y + m * N + n) = v;
  }
}

// ---------------------------------------------------------------- large-tile variant
// For the big MFMA-bound shapes (BERT: M = B*128, N >= 768, K >= 768; Swin stage 3-4): 512
// threads = 8 waves (WM x WN), wave tile (MT*16) x (NT*16), workgroup tile TBM x TBN (256 x 256
// or 256 x 128), one workgroup per CU, 2 waves per SIMD.  K is staged in KB-deep slices through
// a STAGES-deep LDS ring filled by glds (source-swizzled, lane-linear per wave instruction);
// STAGES-2 slices stay in flight across each barrier (counted vmcnt + raw s_barrier —
// __syncthreads would drain them, cdna_hip_programming.md §5 "Pipelining across barriers").

template <int KB>
__device__ __forceinline__ int swzk(int row, int chunk) {
  return KB == 64 ? (chunk ^ ((row >> 1) & 7)) : (chunk ^ ((row >> 1) & 3));  // conflict-free b128 reads
}

// Epilogue of the 8-wave kernels (wave tile MT*16 x NT*16 at (wm, wn)): in 64-row halves of the
// wave tile through LDS (bf16), 16-B row stores (measured: 8-B register-direct stores of a C^T
// product are 15-20 % slower on these shapes).  Starts with a block barrier (the LDS stages are
// reused as staging).
// ROWS: rows of the wave tile staged per round (64, or 32 when the staging must fit in one free
// LDS stage); SYNC: open with __syncthreads (else the caller has already made dsm free).
template <int MT, int NT, int ACT, bool HAS_BIAS, bool HAS_RES, int ROWS = 64, bool SYNC = true>
__device__ __forceinline__ void big_epilogue(f32x4 (&acc)[MT][NT], uint16_t* dsm, const float* __restrict__ bias,
                                             const uint16_t* __restrict__ R, uint16_t* __restrict__ Y,
                                             int64_t M, int N, int64_t m0, int n0, int wm, int wn, int wave,
                                             int lane) {
  const int fr = lane & 15, fq = lane >> 4;
  constexpr int HALVES = MT * 16 / ROWS, MPH = ROWS / 16;  // staging rounds, m-tiles per round
  constexpr int CPR = NT * 16 / 8;  // 16-B chunks per row of the wave tile
  // residual rows are fetched first, so their latency overlaps the LDS staging below
  constexpr int NIT = (ROWS * CPR + 63) / 64;  // 16-B chunks per lane per staging round
  bf16x8 rres[HAS_RES ? HALVES : 1][HAS_RES ? NIT : 1];
  if constexpr (HAS_RES) {
#pragma unroll
    for (int hh = 0; hh < HALVES; ++hh)
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        const int c = it * 64 + lane;
        const int64_t m = m0 + wm * MT * 16 + hh * ROWS + c / CPR;
        const int n = n0 + wn * NT * 16 + (c % CPR) * 8;
        // unconditional (clamped; out-of-range values are never stored): a "load or zero" makes hipcc
        // wait for each residual load before issuing the next
        const int64_t mc = m < M ? m : M - 1;
        const int nc = n < N ? n : N - 8;
        rres[hh][it] = *(const bf16x8*)(R + mc * N + nc);
      }
#pragma unroll
    for (int hh = 0; hh < HALVES; ++hh)
#pragma unroll
      for (int it = 0; it < NIT; ++it) mmr::pin(rres[hh][it]);
  }
  f32x4 bvs[NT];  // bias of the wave's columns, all loads issued at once
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int n = n0 + wn * NT * 16 + j * 16 + fq * 4;
    bvs[j] = HAS_BIAS ? *(const f32x4*)(bias + (n < N ? n : N - 4)) : (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  if constexpr (SYNC) __syncthreads();
  uint16_t* et = dsm + wave * ROWS * EPI_LD;
#pragma unroll
  for (int hh = 0; hh < HALVES; ++hh) {
    // C^T tiles (operands swapped): lane has row m = 16i + (l&15), columns 16j + 4(l>>4) + 0..3
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int nl = j * 16 + fq * 4;
      const f32x4 bv = bvs[j];
      const float bb[4] = {bv[0], bv[1], bv[2], bv[3]};
#pragma unroll
      for (int i4 = 0; i4 < MPH; ++i4) {
        float v[4];
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
          v[rg] = acc[hh * MPH + i4][j][rg] + bb[rg];
          if (ACT == 1) v[rg] = mmr::gelu_fast(v[rg]);
        }
        uint2 pk;
        pk.x = mmr::pack2bf(v[0], v[1]);
        pk.y = mmr::pack2bf(v[2], v[3]);
        *(uint2*)(et + (i4 * 16 + fr) * EPI_LD + nl) = pk;
      }
    }
    __builtin_amdgcn_s_waitcnt(LGKM0);
    __builtin_amdgcn_wave_barrier();
    // all LDS reads of the round first (unconditional; a read under the store's range test makes
    // hipcc wait for each one before the next), then the guarded stores
    bf16x8 vv[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int c = it * 64 + lane;
      const int rl = c / CPR < ROWS ? c / CPR : ROWS - 1, cc = (c % CPR) * 8;
      vv[it] = *(const bf16x8*)(et + rl * EPI_LD + cc);
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int c = it * 64 + lane;
      const int rl = c / CPR, cc = (c % CPR) * 8;
      const int64_t m = m0 + wm * MT * 16 + hh * ROWS + rl;
      const int n = n0 + wn * NT * 16 + cc;
      if (c >= ROWS * CPR || m >= M || n >= N) continue;
      bf16x8 v = vv[it];
      if (HAS_RES) {
        const bf16x8 rr = rres[HAS_RES ? hh : 0][HAS_RES ? it : 0];
        uint32_t o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e)
          o[e] = mmr::pack2bf(mmr::bf2f((uint16_t)v[2 * e]) + mmr::bf2f((uint16_t)rr[2 * e]),
                              mmr::bf2f((uint16_t)v[2 * e + 1]) + mmr::bf2f((uint16_t)rr[2 * e + 1]));
        v = __builtin_bit_cast(bf16x8, make_uint4(o[0], o[1], o[2], o[3]));
      }
      *(bf16x8*)(Y + m * N + n) = v;
    }
    __builtin_amdgcn_wave_barrier();
  }
}

template <int WM, int WN, int MT, int NT, int KB, int STAGES, int ACT, bool HAS_BIAS, bool HAS_RES,
          int OCC = 1>
__global__ __launch_bounds__(512, 2 * OCC) void gemm_bf16_tn_big(const uint16_t* __restrict__ X,
                                                           const uint16_t* __restrict__ W,
                                                           const float* __restrict__ bias,
                                                           const uint16_t* __restrict__ R,
                                                           uint16_t* __restrict__ Y, int64_t M,
                                                           int N, int K, int tiles_m, int tiles_n) {
  constexpr int TBM = WM * MT * 16, TBN = WN * NT * 16;
  constexpr int CH = KB / 8;                 // 16-B chunks per LDS row
  constexpr int RPI = 64 / CH;               // rows per glds wave instruction (1 KiB)
  constexpr int TA = TBM * KB, TB = TBN * KB;  // bf16 elements per stage
  constexpr int CA = TBM * CH / 512, CB = TBN * CH / 512;  // glds per thread per operand
  constexpr int KS = KB / 32;                // 32-deep MFMA k-steps per slice
  extern __shared__ __attribute__((aligned(16))) uint16_t dsm[];  // [STAGES][TA + TB]

  const int nwg = tiles_m * tiles_n;
  const int orig = blockIdx.x;
  const int q = nwg / 8, r8 = nwg % 8, xcd = orig % 8;
  const int wg = (xcd < r8 ? xcd * (q + 1) : r8 * (q + 1) + (xcd - r8) * q) + orig / 8;
  const int tm = wg / tiles_n, tn = wg % tiles_n;
  const int64_t m0 = (int64_t)tm * TBM;
  const int n0 = tn * TBN;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;

  const int prow_in = lane / CH, pch = lane % CH;
  const uint16_t* srcA[CA];
  const uint16_t* srcB[CB];
  int lcA[CA], lcB[CB];
#pragma unroll
  for (int j = 0; j < CA; ++j) {
    const int row = RPI * (wave + 8 * j) + prow_in;
    lcA[j] = swzk<KB>(row, pch) * 8;
    const int64_t gm = m0 + row;
    srcA[j] = gm < M ? X + gm * K : nullptr;
  }
#pragma unroll
  for (int j = 0; j < CB; ++j) {
    const int row = RPI * (wave + 8 * j) + prow_in;
    lcB[j] = swzk<KB>(row, pch) * 8;
    const int gn = n0 + row;
    srcB[j] = gn < N ? W + (int64_t)gn * K : nullptr;
  }
  const uint16_t* zp = (const uint16_t*)g_zero_page;
  // one glds piece (1 KiB per wave): pieces 0..CA-1 stage A, CA..CA+CB-1 stage B
  auto stage_piece = [&](int s, int k0, int p) {
    uint16_t* la = dsm + s * (TA + TB);
    if (p < CA) {
      const int k = k0 + lcA[p];
      const uint16_t* a = (srcA[p] && k < K) ? srcA[p] + k : zp;
      __builtin_amdgcn_global_load_lds((const void*)a, (lds_ptr_t)(la + RPI * (wave + 8 * p) * KB), 16, 0, 0);
    } else {
      const int j = p - CA;
      const int k = k0 + lcB[j];
      const uint16_t* b = (srcB[j] && k < K) ? srcB[j] + k : zp;
      __builtin_amdgcn_global_load_lds((const void*)b, (lds_ptr_t)(la + TA + RPI * (wave + 8 * j) * KB), 16, 0, 0);
    }
  };
  auto stage = [&](int s, int k0) {
#pragma unroll
    for (int p = 0; p < CA + CB; ++p) stage_piece(s, k0, p);
  };

  f32x4 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int nk = (K + KB - 1) / KB;
  const int fr = lane & 15, fq = lane >> 4;
  constexpr int PER_TILE = CA + CB;
#pragma unroll
  for (int p = 0; p < STAGES - 1; ++p)
    if (p < nk) stage(p, p * KB);
  for (int kt = 0; kt < nk; ++kt) {
    const int after = min(STAGES - 2, nk - 1 - kt);  // slices issued after kt allowed in flight
    if (STAGES >= 4 && after >= 2) {
      if (STAGES >= 5 && after >= 3) __builtin_amdgcn_s_waitcnt(vmcnt_n(3 * PER_TILE));
      else __builtin_amdgcn_s_waitcnt(vmcnt_n(2 * PER_TILE));
    } else if (STAGES >= 3 && after >= 1) {
      __builtin_amdgcn_s_waitcnt(vmcnt_n(PER_TILE));
    } else {
      __builtin_amdgcn_s_waitcnt(vmcnt_n(0));
    }
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    const bool more = kt + STAGES - 1 < nk;
    const int s_next = (kt + STAGES - 1) % STAGES, k_next = (kt + STAGES - 1) * KB;
    const int s = kt % STAGES;
    const uint16_t* la = dsm + s * (TA + TB);
    const uint16_t* lb = la + TA;
    auto rdA = [&](int ks, int i) {
      const int rowa = wm * MT * 16 + i * 16 + fr;
      return *(const bf16x8*)(la + rowa * KB + swzk<KB>(rowa, ks * 4 + fq) * 8);
    };
    auto rdB = [&](int ks, int j) {
      const int rowb = wn * NT * 16 + j * 16 + fr;
      return *(const bf16x8*)(lb + rowb * KB + swzk<KB>(rowb, ks * 4 + fq) * 8);
    };
    if (KS == 2 && MT == 8 && NT <= 4 && CA + CB <= MT) {
      // hand-placed interleave (glds are scheduling barriers for hipcc, so source order holds):
      // k-step-0 fragments; then per A row-tile i: one glds piece of the next slice, the
      // k-step-1 fragment(s), 4 k-step-0 MFMAs; then the 32 k-step-1 MFMAs.
      bf16x8 a0[MT], b0[NT], a1[MT], b1[NT];
#pragma unroll
      for (int j = 0; j < NT; ++j) b0[j] = rdB(0, j);
#pragma unroll
      for (int i = 0; i < MT; ++i) a0[i] = rdA(0, i);
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        if (more && i < CA + CB) stage_piece(s_next, k_next, i);
        a1[i] = rdA(1, i);
        if (i < NT) b1[i] = rdB(1, i);
#pragma unroll
        for (int j = 0; j < NT; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b0[j], a0[i], acc[i][j], 0, 0, 0);
      }
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b1[j], a1[i], acc[i][j], 0, 0, 0);
    } else {
      if (more) stage(s_next, k_next);
      bf16x8 a[KS][MT], b[KS][NT];
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
        for (int j = 0; j < NT; ++j) b[ks][j] = rdB(ks, j);
#pragma unroll
        for (int i = 0; i < MT; ++i) a[ks][i] = rdA(ks, i);
      }
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int j = 0; j < NT; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[ks][j], a[ks][i], acc[i][j], 0, 0, 0);
      if (KS == 2) {
        __builtin_amdgcn_sched_group_barrier(0x100, MT + NT, 0);
#pragma unroll
        for (int g = 0; g < MT + NT; ++g) {
          __builtin_amdgcn_sched_group_barrier(0x008, MT * NT / (MT + NT) > 0 ? MT * NT / (MT + NT) : 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x008, 2 * MT * NT, 0);
      }
    }
    __builtin_amdgcn_s_waitcnt(LGKM0);  // lgkmcnt(0): this slice's fragment reads returned
  }

  big_epilogue<MT, NT, ACT, HAS_BIAS, HAS_RES>(acc, dsm, bias, R, Y, M, N, m0, n0, wm, wn, wave, lane);
}


// ---------------------------------------------------------------- 8-phase persistent 256 x 64NT GEMM
// cdna_hip_programming.md §5 "256² 8-phase template" (T1-T5), re-derived for nn.Linear operands and
// made persistent: 8 waves = 2 (M) x 4 (N), wave tile 128 x 16NT (NT = 4: 256 x 256, NT = 3:
// 256 x 192), BK = 64, two LDS K-tile buffers E / O (even / odd K-tile), each [A 256 x 64 | B 64NT x
// 64] bf16, source-swizzled glds pieces (one wave instruction = 8 rows x 128 B; piece j of an
// operand = its rows 64j..64j+63).
// A K-tile is 4 phases; phase q computes one quadrant of the wave tile (m-half x n-half, both
// k-steps) from fragments read in the phase's load segment:
//   q0: read A[mh0], B[nh0] -> MFMA (mh0, nh0)      q1: read B[nh1] -> MFMA (mh0, nh1)
//   q2: read A[mh1] -> MFMA (mh1, nh1)              q3: -> MFMA (mh1, nh0)
// Each phase = load segment | s_barrier | MFMA segment | s_barrier; waves 4-7 (m-group 1) run one
// barrier behind waves 0-3, so on every SIMD one wave's MFMA segment overlaps its partner's
// LDS-read / glds segment (MI355X_MICROARCH.md "Two waves per SIMD").
// glds schedule by segment s = 0..15 of an iteration (2 K-tiles; s = 2p load, 2p+1 MFMA segment
// of phase p), each region re-staged only after every reader retired it (a barrier after the later
// group's lgkmcnt):  E.A0 s2, E.A2 s3, E.B0 s5, E.B1+E.A1 s6, E.B2+E.A3 s7, E.B3 s8, and the same
// + 8 for O.  Waits: vmcnt(5) at the end of s6 (O complete before group 0 reads it at s8) and s14
// (E before s16): 5 younger pieces stay in flight across each wait.
// Persistent: one workgroup per CU walks its XCD's tiles (consecutive tiles share the X panel in
// that XCD's L2).  The K-tile stream runs on across tiles — the last iteration of a tile loads the
// next tile's K-tiles 0 and 1 — so there is no per-tile prologue burst; the epilogue (bias / GELU /
// residual in f32 -> bf16 -> 16-B row stores) stages through a per-wave LDS area outside E / O
// while those loads are in flight, and the first wait of the next tile counts its stores out
// (vmcnt(5 + NSTORE)) instead of draining them.  M % 256 == 0 (launcher): every store is issued, so
// the count is exact.
// LDS store the compiler does not track: hipcc waits vmcnt(0) before a ds_write that may alias an
// in-flight LDS-DMA, which would drain the next tile's operand loads at the start of every epilogue
__device__ __forceinline__ void ds_write_b64_untracked(const void* p, uint32_t lo, uint32_t hi) {
  const uint32_t a = (uint32_t)(uintptr_t)p;
  const unsigned long long d = ((unsigned long long)hi << 32) | lo;
  asm volatile("ds_write_b64 %0, %1" ::"v"(a), "v"(d) : "memory");
}
__device__ __forceinline__ void ds_write_b128_untracked(const void* p, uint4 v) {
  const uint32_t a = (uint32_t)(uintptr_t)p;
  asm volatile("ds_write_b128 %0, %1" ::"v"(a), "v"(__builtin_bit_cast(u32x4, v)) : "memory");
}

typedef int i32x8 __attribute__((ext_vector_type(8)));
// v_mfma_scale_f32_16x16x128_f8f6f4, e4m3 x e4m3; scale bytes selected by (compile-time) opsel
__device__ __forceinline__ f32x4 mx_mfma(i32x8 a, i32x8 b, f32x4 c, uint32_t sa, int ja, uint32_t sb, int jb) {
#define MX_CASE(A, B) \
  if (ja == A && jb == B) return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 0, 0, A, (int)sa, B, (int)sb);
  MX_CASE(0, 0) MX_CASE(0, 1) MX_CASE(0, 2) MX_CASE(0, 3) MX_CASE(1, 0) MX_CASE(1, 1) MX_CASE(1, 2) MX_CASE(1, 3)
  MX_CASE(2, 0) MX_CASE(2, 1) MX_CASE(2, 2) MX_CASE(2, 3) MX_CASE(3, 0) MX_CASE(3, 1) MX_CASE(3, 2) MX_CASE(3, 3)
#undef MX_CASE
  return c;
}

// 16-B output store of the 8-phase GEMM epilogue; nt: non-temporal (streamed past L2).  The launchers
// set it for outputs larger than the 256 MB MALL written as whole 128-B lines (the LDS-staged and
// OUT8 epilogues): the output then no longer evicts the X / W panels the concurrent tiles re-read
// (random operands, M = 262144: fp8 QKV 1551 -> 1940 TF, O 1537 -> 1849, Swin qkv +29 %; bf16 QKV
// +4 %).  The permlane epilogue writes 64-B half lines and stays write-back (non-temporal: bf16 FFN1
// -10 %), as do outputs the next kernel may find in the MALL.  profiles/r03_p8_nt_store_ab.txt.
__device__ __forceinline__ void st16(void* p, uint4 v, bool nt) {
  if (nt) __builtin_nontemporal_store(__builtin_bit_cast(u32x4, v), (u32x4*)p);
  else *(uint4*)p = v;
}

// the launchers' choice: outputs above 128 MB stream (the cfg2 BERT / fusion QKV outputs, 151 MB:
// QKV 121 -> 118.5 us, step 15.58 -> 15.51 ms same box, profiles/r03_s4_nt_store_step.txt); the 50 MB
// O / FFN2 outputs measured equal
inline int p8_nt(int64_t m, int64_t n, int64_t esz) { return m * n * esz > (int64_t)128 << 20 ? 1 : 0; }

template <int NT, bool FP8 = false, int KNN = 0, int NV = 1>
struct P8 {
  static constexpr int TBN = 64 * NT;
  // NV: per-column f32 vectors staged per tile (bias; + the LayerNorm-fold vectors, see LNM)
  static constexpr int SC = FP8 ? 1024 : 0;            // uint16 elements of per-K-tile scales (2 KB)
  static constexpr int RM = NT == 3 ? 2 : 1;           // m-tiles per epilogue round
  static constexpr int ELD = 16 * NT + 8;              // bf16 row stride of the epilogue area
  static constexpr int CPL = 16 * RM * 2 * NT / 64;    // 16-B chunks per lane per round
  // global stores per wave per tile (KNN: 8 m-tiles x (4 unit-max + 1 block-max) stores; the LDS-
  // staged epilogue (OUT8, MMR_P8_EPI=0): 8 / RM rounds x CPL 16-B chunks; the permlane epilogue:
  // one 16-B store per (m-tile, n-tile pair) — NT = 3 stores its odd tile as a pair with itself)
  // (KNN: staging the 2-row unit maxima through LDS into 64-B row segments — 24 stores instead of
  // 40 — measured 59.3 -> 61.7 us at Q=256 x 100k: the round trips cost more than the store path
  // saves; without any unit-maxima stores the scan runs 46 us, profiles/r03_knn_unit_store_ab.txt)
  static constexpr int NSTORE_LDS = KNN ? 40 : (8 / RM) * CPL;
  static constexpr int NSTORE_PL = 8 * ((NT + 1) / 2);
  static constexpr size_t BUF_B = (size_t)(256 + TBN) * 64 * 2 + SC * 2;
  static constexpr size_t EPI_B = 8ull * 16 * RM * ELD * 2;
#ifdef MMR_P8_STAMPS
  static constexpr size_t STAMP_B = 8 * 8 * 4 * 8;  // diagnostic build: [wave][tile < 8][4] u64 clocks
#else
  static constexpr size_t STAMP_B = 0;
#endif
  static constexpr size_t COEF_B = NV > 1 ? 2 * 256 * 2 * 4 : 0;  // LNM: [2][256 rows][rstd, -mean rstd]
  static constexpr size_t LDS_B = 2 * BUF_B + EPI_B + 2 * NV * TBN * 4 + COEF_B + STAMP_B;
};

#ifdef MMR_P8_STAMPS
// Diagnostic build only (tools/p8_stamps.py): per workgroup, wave and tile (first 8 tiles) the shader
// clock at the tile's start, at the end of its K loop and at the end of its epilogue, plus the
// 100 MHz real-time clock at the tile start — buffered in LDS (no vmcnt traffic in the loop),
// written out at the kernel's end.
__device__ unsigned long long p8_stamps[1024 * 8 * 8 * 4];
#endif

// FP8 = true: the MX-fp8 form (OCP e4m3 operands, one E8M0 scale per 32 consecutive k of a row;
// gfx950 v_mfma_scale_f32_16x16x128_f8f6f4).  A K-tile is then 128 k = the same 128-byte LDS rows,
// one MFMA per (m-tile, n-tile) instead of two; X / W are byte matrices with row stride K, the
// scales (XS, WS) are pre-arranged by mmr_quantize_mxfp8 in the per-lane order of the LDS scale
// image (1 KB per operand panel and K-tile), staged by one more LDS-DMA each.  Fragment map
// (tools/mfma_fp8_probe.hip, exact on integer data): lane (r = l%16, g = l/16) holds k = 16g..16g+15
// and 64+16g..64+16g+15 of row r — the two 16-byte chunks the bf16 form reads as k-steps 0 / 1 —
// and supplies the scale of row r, k-block g.
// OUT8 (FP8, NT = 4, no residual): the output is written as the NEXT GEMM's MX-fp8 activation
// operand — e4m3 bytes [M][N] (Y reinterpreted) + E8M0 scales in the layout-0 image (YS) — instead of
// bf16: each lane takes 16 values of one staged bf16 row, the 32-block max is one lane swap, so the
// result is bit-identical to mmr_quantize_mxfp8 of the bf16 output (same per-round store count).
// KNN (NT = 4, no bias / residual / act): the fp16 cosine scan of knn.hip (mmr::knn_scan_p8) — X =
// the <= 256 fp16 unit queries [256][K], W = the fp16 unit gallery rows [tiles_n * 256][K], fp16 MFMA
// (v_mfma_f32_16x16x32_f16: exact products, f32 accumulate).  The C^T layout gives a lane 4
// CONSECUTIVE gallery rows of one query, so the epilogue stores the maxima of its two row pairs
// (KNN = 2: knn_select_t<3>'s 2-row units, one 8-B store) or of all four (KNN = 4: knn_select_t<2>'s
// 4-row units) — GM[q][unit] (ldG) — and each wave column's 64-row block max BM[q][block] (ldB),
// rows >= nval as -inf, instead of the tile.
// LNM / STO (bf16, 256-row tiles): the BERT residual + LayerNorm folded into the GEMMs around it, so
// no LayerNorm pass runs between them (mmr_linear_bf16_ln).  A producer (STO) writes, besides its
// bf16 output y, one (sum y, M2 = sum (y - part mean)^2) f32 pair per row, tile column and wave column
// (a part of 16 NT columns) — SP[row][4 n-tile + wc], over the bf16-ROUNDED outputs (deterministic, no
// atomics); mmr_ln_row_coef merges the parts by Chan's formula.  A consumer reads the LP pairs of
// input rows, reduced by mmr_ln_row_coef to LC[row] = (rstd, -mean rstd) — staged per tile into LDS
// by LDS-DMA beside the bias (a global load in the epilogue would retire behind the next tile's
// prefetch and expose it) — and either
//   LNM = 1: takes the raw y as X and applies LN(y) W^T + b = rstd (y W'^T) - rstd mean c + d in the
//            epilogue (W' = W diag(gamma) pre-folded, LV1 = c = row sums of W', bias = d = W beta + b);
//   LNM = 2: takes the raw y as the residual R and adds LN(y) = gamma (rstd y - rstd mean) + beta
//            (LV1 = gamma, LV2 = beta over the output columns).
#ifndef MMR_X3_PRODUCTS
#define MMR_X3_PRODUCTS 3
#endif
#ifndef X3ST_AUX
#define X3ST_AUX 0
#endif
template <int NT, int ACT, bool HAS_BIAS, bool HAS_RES, bool FP8 = false, bool OUT8 = false, int KNN = 0,
          int LNM = 0, bool STO = false, bool OF32 = false, bool OSPL = false, bool X3P = false>
__global__ __launch_bounds__(512) void gemm_bf16_tn_p8(const uint16_t* __restrict__ X,
                                                       const uint16_t* __restrict__ W,
                                                       const float* __restrict__ bias,
                                                       const uint16_t* __restrict__ R,
                                                       uint16_t* __restrict__ Y, int64_t M, int N,
                                                       int K, int tiles_m, int tiles_n,
                                                       const uint8_t* __restrict__ XS = nullptr,
                                                       const uint8_t* __restrict__ WS = nullptr,
                                                       uint8_t* __restrict__ YS = nullptr,
                                                       float* __restrict__ GM = nullptr, float* __restrict__ BM = nullptr,
                                                       int64_t ldG = 0, int64_t ldB = 0, int64_t nval = 0,
                                                       int ntst = 0, const float* __restrict__ RS = nullptr,
                                                       const float* __restrict__ LC = nullptr,
                                                       const float* __restrict__ LV1 = nullptr,
                                                       const float* __restrict__ LV2 = nullptr,
                                                       float* __restrict__ SP = nullptr, int ldn = 0) {
  static_assert(!OUT8 || (FP8 && NT == 4 && !HAS_RES), "OUT8: MX-fp8 256x256 tiles without residual");
  static_assert((LNM == 0 && !STO) || (!FP8 && !KNN), "LayerNorm fold: bf16 GEMMs");
  static_assert(LNM != 2 || HAS_RES, "LNM = 2 normalises the residual");
  static_assert(!STO || ACT == 0, "row statistics: LDS-staged (non-GELU) epilogue");
  static_assert(!OF32 || (!FP8 && !OUT8 && !KNN && LNM == 0 && !STO), "f32 output: plain bf16 operands");
  // OSPL (with OF32): the output written as the next x3 GEMM's split operand rows [hi | lo] (bf16, row
  // width 2 N) instead of f32 — one 8-B store of each per (m-tile, n-tile)
  static_assert(!OSPL || (OF32 && NT == 3 && !HAS_RES), "split output: OF32 256 x 192 tiles without residual");
  static_assert(!X3P || OF32, "three-product split operands: the x3 split GEMM (f32 output)");
  static_assert(KNN == 0 || ((KNN == 2 || KNN == 4) && NT == 4 && !FP8 && !HAS_BIAS && !HAS_RES && ACT == 0),
                "KNN (rows per unit 2 / 4): plain 256x256 fp16 tiles");
#if defined(__HIP_DEVICE_COMPILE__)  // buffer-descriptor builtins exist in the device pass only
  constexpr int NV = LNM == 2 ? 3 : (LNM == 1 ? 2 : 1);
  using C = P8<NT, FP8, KNN, NV>;
  constexpr int KB = 64, TBN = C::TBN;                  // KB: 128-byte LDS rows (64 bf16 / 128 fp8)
  constexpr int TA = 256 * KB, TB = TBN * KB, BUF = TA + TB + C::SC;  // uint16 elements per K-tile buffer
  // LDS image: [A_E | A_O | B_E | B_O | S_E | S_O] — the two buffers of an operand 32 KB apart, so one
  // base register per (operand, k-step) reaches both through the ds_read immediate offset
  auto aoff = [](int buf) { return buf * TA; };
  auto boff = [](int buf) { return 2 * TA + buf * TB; };
  auto soff = [](int buf) { return 2 * (TA + TB) + buf * C::SC; };
  constexpr int ESZ = FP8 ? 1 : 2;                      // operand element bytes
  constexpr int NH0 = NT / 2;                           // n-tiles in n-half 0
  // Residual of bf16 NT = 3 tiles with the LDS-staged epilogue: loaded at the START of the tile as
  // 16-B row chunks (the layout the epilogue stores in; 12 loads per lane into 48 VGPRs, held through
  // the K loop) and turned into the fragment layout through the wave's LDS epilogue area, instead of
  // 24 x 8-B fragment-layout loads in the epilogue (16 half-used lines per load instruction, and an
  // epilogue load retires — vmcnt, in order — behind the next tile's K-tile prefetch).  The tile's
  // first counted wait leaves them in flight (NRES more younger ops).  NT = 4 / FP8 tiles have no
  // registers for them.
  constexpr bool early_res = HAS_RES && NT == 3 && !FP8 && !OF32 && !(!OUT8 && !KNN && ACT == 1);
  constexpr int NRES = early_res ? (8 / C::RM) * C::CPL : 0;
  static_assert(C::NSTORE_LDS + 13 + NRES <= 63 && C::NSTORE_PL + 5 + NRES <= 63, "vmcnt range");
  // Epilogue: permlane row chunks straight from registers (no LDS round trips) for GELU epilogues,
  // the per-wave LDS staging otherwise: measured (random operands, profiles/r03_gemm_epilogue_ab.txt)
  // FFN1 + GELU 925 -> 1015 TF and Swin fc1 + GELU +8 % with permlane, but the plain / residual
  // epilogues 3-7 % slower than with the LDS path (QKV 1041 vs 947 TF at 256 x 192: its 16 rows x
  // 64 B stores are twice the L2 write requests of the LDS path's 8 rows x 128 B).  OUT8 / KNN keep
  // their own epilogues.
  constexpr bool epi_pl = !OUT8 && !KNN && !OF32 && ACT == 1;
  // (OUT8 + GELU in registers — permlane row chunks quantised after two lane swaps — measured slower
  // than the LDS-staged OUT8 rounds and was removed: profiles/r03_out8_permlane_ab.txt)
#ifdef MMR_P8_NOSTORE
  constexpr bool skip_st = !KNN && !OUT8;  // diagnostic build: bf16 outputs computed, not stored
  constexpr bool skip_gm = KNN != 0;       // ... and the kNN unit maxima (block maxima still stored)
#else
  constexpr bool skip_st = false;
  constexpr bool skip_gm = false;
#endif
  // STO: 8 more (one row-statistics store per m-tile, lanes fq = 0 — the instruction always issues)
  // OF32: one 16-B store per (m-tile, n-tile) straight from the accumulators; OSPL: two (hi, lo) per (m-tile,
  // n-tile pair)
  constexpr int nstore = skip_st ? 0
                                 : (OF32 ? (NT == 3 ? 24 : (OSPL ? 16 * ((NT + 1) / 2) : 8 * NT))
                                         : (skip_gm ? 8 : (epi_pl ? C::NSTORE_PL : C::NSTORE_LDS) + (STO ? 8 : 0)));
  static_assert(!OF32 || (OSPL ? 16 * ((NT + 1) / 2) : 8 * NT) + 5 <= 63, "vmcnt range");
  extern __shared__ __attribute__((aligned(16))) uint16_t dsm[];

  const int ntiles = tiles_m * tiles_n;
  const int per = gridDim.x / 8, xcd = blockIdx.x % 8, slot = blockIdx.x / 8;
  // Tile order: the XCD's share is a contiguous run of the row-major (m, n) tile grid (the 32
  // concurrent tiles of an XCD share X panels; W panels are re-read from the MALL once per round of
  // concurrent tiles).  An n-chunked order that keeps a slice of W resident in the XCD's L2 (W read
  // once per XCD) measured 1-6 % slower on every BERT shape (profiles/r03_gemm_tile_order_ab.txt).
  const int lo = (int)((int64_t)ntiles * xcd / 8), hi = (int)((int64_t)ntiles * (xcd + 1) / 8);
  int t = lo + slot;
  if (t >= hi) return;
  // KNN: query tile fastest (tiles_m = 1 or 2), so the two query tiles of a gallery tile run at once
  // on CUs of one XCD and the second reads the gallery panel from its L2
  auto mof = [&](int tile) -> int { return KNN ? tile % tiles_m : tile / tiles_n; };
  auto nof = [&](int tile) -> int { return KNN ? tile / tiles_m : tile % tiles_n; };

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // provably uniform: SGPR LDS bases
  const int wr = wave >> 2, wc = wave & 3;  // m-group (stagger group), n position
  const int fr = lane & 15, fq = lane >> 4;
  uint16_t* et = dsm + 2 * BUF + wave * 16 * C::RM * C::ELD;         // this wave's epilogue area
  float* lbias = (float*)(dsm + 2 * BUF + 8 * 16 * C::RM * C::ELD);  // [2][NV][TBN] f32, by tile parity
  // bias (and LNM vectors) of a tile -> LDS by LDS-DMA from wave 0: the first tile's in the prologue,
  // each next tile's at the end of wave 0's epilogue (the other parity; no registers live across the loop)
  float* lcoef = lbias + 2 * NV * TBN;  // LNM: [2][256][2] f32 row coefficients, by tile parity
  // (buffer-descriptor form: uniform bases in SGPRs, the lane's byte offset recomputed from an opaque
  // lane id — a 64-bit per-lane address kept live across the loop was spilled in the MX-fp8 kernels,
  // and its reload, a vmcnt op, drained the next tile's prefetch at every tile)
  auto bias_dma = [&](int tile, int par) {
    if (wave != 0) return;
    int ll;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ll));
    const uint32_t lo16 = (uint32_t)ll * 16;
    auto dma = [&](const float* base, float* dst, int soff) {
      const auto rs = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, 0x7FFFFFFF, 0x00020000);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_ptr_t)dst, 16, lo16, soff, 0, 0);
    };
    if (LNM != 0) {  // the tile's 256 row-coefficient pairs: 2 x 1 KB
      const float* src = LC + (int64_t)mof(tile) * 512;
      dma(src, lcoef + par * 512, 0);
      dma(src, lcoef + par * 512 + 256, 1024);
    }
    if (ll < TBN / 4) {
      if (HAS_BIAS) dma(bias + nof(tile) * TBN, lbias + par * NV * TBN, 0);
      // KNN over a raw-row gallery (the native fp16 index): the tile's 256 per-row 1 / |g| in the bias slot
      if (KNN && RS != nullptr) dma(RS + nof(tile) * TBN, lbias + par * NV * TBN, 0);
      if (LNM != 0) dma(LV1 + nof(tile) * TBN, lbias + (par * NV + 1) * TBN, 0);
      if (LNM == 2) dma(LV2 + nof(tile) * TBN, lbias + (par * NV + 2) * TBN, 0);
    }
  };

  // glds: piece j of an operand stages LDS rows 64j + 8 wave + lane/8, physical chunk lane%8 <-
  // logical chunk swz(row, lane%8); per-lane byte offsets are tile-independent, a tile contributes
  // uniform bases only
  // piece j's rows are 64 j + (piece 0's rows) and the swizzle depends on (row >> 1) & 7 only, so
  // one per-lane offset serves every piece of an operand: 64 j rows go into the uniform soffset
  const int prow = lane >> 3, pch = lane & 7;
  const int row0 = 8 * wave + prow;
  // X3P (the x3 split GEMM): X and W rows are [hi | lo] bf16, each segment kp = K / 2 wide, and one K-tile
  // is 32 k of BOTH: LDS row = [hi 32 k | lo 32 k] (logical chunks 0-3 hi, 4-7 lo), so k-step 0 reads the
  // hi fragment and k-step 1 the lo fragment of the same 32 k, and the MFMA segment issues hi.hi, lo.hi and
  // hi.lo from those four fragments — each operand staged once (no [w_hi | w_lo | w_hi] image, no x_hi
  // re-read) and 3 MFMAs per (m-tile, n-tile) per fragment set instead of 2.  A logical chunk c >= 4 sits
  // kp elements (K bytes) further along the row; a K-tile advances 64 bytes.
  auto chb = [&](int c) { return X3P ? (c < 4 ? c * 16 : K + (c - 4) * 16) : c * 16; };
  const uint32_t off0 = (uint32_t)(row0 * K * ESZ + chb(swz(row0, pch)));
  const uint32_t pstride = (uint32_t)(64 * K * ESZ);  // bytes between consecutive pieces of an operand
  constexpr int KTX = X3P ? 64 : KB * 2;              // X bytes per K-tile
  // KNN: the gallery W is in the index's tile32h layout (16-row x 32-half 1-KB pieces, knn.hip
  // tile32h_index) — the same image every other fp16 scan reads, so the index keeps ONE fp16 copy.
  // Logical chunk c of row r in K-tile kt = piece (r/16, 2 kt + c/4), lane slot (c%4) 16 + r%16: the
  // per-lane offset is fixed, a K-tile adds 2 KB (uniform soffset), and 64 rows are still pstride.
  const int wch = swz(row0, pch);
  const uint32_t off0w = KNN ? (uint32_t)(((row0 >> 4) * (K / 32) + (wch >> 2)) * 1024 + (((wch & 3) << 4) + (row0 & 15)) * 16)
                             : off0;
  constexpr int KTW = KNN ? 2048 : KTX;  // W bytes per K-tile
  const int nk = K * ESZ / 128;  // 128-byte K-tiles (X3P: 2 x 64 bytes); even (launcher)
  // operand panels as buffer descriptors (uniform, SGPRs): a piece is buffer_load ... lds with the
  // per-lane offset in voffset and the K-tile offset in soffset — no per-piece address registers
#ifdef MMR_P8_SAMEPANEL
  // diagnostic build: every tile stages the FIRST X / W panels (L2-resident operand stream; results wrong)
  auto pan = [](int) { return 0; };
#else
  auto pan = [](int v) { return v; };
#endif
  auto xbase = [&](int tile) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)X + (int64_t)pan(mof(tile)) * 256 * K * ESZ), 0, 0x7FFFFFFF, 0x00020000);
  };
  auto wbase = [&](int tile) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)W + (int64_t)pan(nof(tile)) * TBN * K * ESZ), 0, 0x7FFFFFFF, 0x00020000);
  };
  // MX scales: one 1-KB piece per operand panel and K-tile (wave 0: X's, wave 1: W's); a wave issues
  // it with its first piece of that K-tile, so every count-based wait below still covers it
  const auto xsr = __builtin_amdgcn_make_buffer_rsrc((void*)XS, 0, 0x7FFFFFFF, 0x00020000);
  const auto wsr = __builtin_amdgcn_make_buffer_rsrc((void*)WS, 0, 0x7FFFFFFF, 0x00020000);
  // a tile's scale-panel base (K-tile 0) in bytes, for wave 0 (X's) / wave 1 (W's) / others (unused);
  // computed once per tile: in the K loop the tile's division would be re-done per K-tile (SALU)
  auto sbase = [&](int tile) -> int {
    return FP8 ? (wave == 0 ? mof(tile) : nof(tile)) * nk * 1024 : 0;
  };
  auto gS = [&](int sb, int buf, int kt) {
    if constexpr (FP8) {
      if (wave < 2) {
        // the lane offset from a freshly computed lane id: held across the K loop, the bias + residual
        // instantiation spilled it, and its reload (a vmcnt op) drained the K-tile prefetch of waves 0 / 1
        int ll;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ll));
        __builtin_amdgcn_raw_ptr_buffer_load_lds(wave == 0 ? xsr : wsr, (lds_ptr_t)(dsm + soff(buf) + wave * 512), 16,
                                                 (uint32_t)ll * 16, sb + kt * 1024, 0, 0);
      }
    }
  };
  auto gA = [&](__amdgpu_buffer_rsrc_t xb, int buf, int j, int kt) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(xb, (lds_ptr_t)(dsm + aoff(buf) + (64 * j + 8 * wave) * KB), 16, off0,
                                             kt * KTX + j * pstride, 0, 0);
  };
  auto gB = [&](__amdgpu_buffer_rsrc_t wb, int buf, int j, int kt) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(wb, (lds_ptr_t)(dsm + boff(buf) + (64 * j + 8 * wave) * KB), 16, off0w,
                                             kt * KTW + j * pstride, 0, 0);
  };
  // fragment reads: the swizzle of row 16i + fr is a function of fr only, so every A (B) fragment
  // address is one of two per-lane bases (k-step 0 / 1: logical chunk fq or 4 + fq) plus an
  // immediate offset (buffer, tile) — 4 + 4 address registers instead of one per fragment
  const int xs = fq ^ ((fr >> 1) & 7);
  const uint16_t* pa[2];
  const uint16_t* pb[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) {
    pa[ks] = dsm + (wr * 128 + fr) * KB + (xs ^ (4 * ks)) * 8;
    pb[ks] = dsm + 2 * TA + (wc * 16 * NT + fr) * KB + (xs ^ (4 * ks)) * 8;
  }
  auto rdA = [&](int buf, int ks, int i) { return *(const bf16x8*)(pa[ks] + buf * TA + i * 16 * KB); };
  auto rdB = [&](int buf, int ks, int j) { return *(const bf16x8*)(pb[ks] + buf * TB + j * 16 * KB); };
  bf16x8 fa[4][2], fb0[NH0][2], fb1[NT - NH0][2];
  i32x8 fa8[4], fb08[NH0], fb18[NT - NH0];  // FP8: the two 16-byte chunks of a fragment, contiguous
  auto ldA = [&](int buf, int i, int mt) {
    if constexpr (FP8) {
      fa8[i] = __builtin_shufflevector(__builtin_bit_cast(i32x4_t, rdA(buf, 0, mt)),
                                       __builtin_bit_cast(i32x4_t, rdA(buf, 1, mt)), 0, 1, 2, 3, 4, 5, 6, 7);
    } else {
      fa[i][0] = rdA(buf, 0, mt);
      fa[i][1] = rdA(buf, 1, mt);
    }
  };
  auto ldB0 = [&](int buf, int j) {
    if constexpr (FP8) {
      fb08[j] = __builtin_shufflevector(__builtin_bit_cast(i32x4_t, rdB(buf, 0, j)),
                                       __builtin_bit_cast(i32x4_t, rdB(buf, 1, j)), 0, 1, 2, 3, 4, 5, 6, 7);
    } else {
      fb0[j][0] = rdB(buf, 0, j);
      fb0[j][1] = rdB(buf, 1, j);
    }
  };
  auto ldB1 = [&](int buf, int j) {
    if constexpr (FP8) {
      fb18[j] = __builtin_shufflevector(__builtin_bit_cast(i32x4_t, rdB(buf, 0, NH0 + j)),
                                       __builtin_bit_cast(i32x4_t, rdB(buf, 1, NH0 + j)), 0, 1, 2, 3, 4, 5, 6, 7);
    } else {
      fb1[j][0] = rdB(buf, 0, NH0 + j);
      fb1[j][1] = rdB(buf, 1, NH0 + j);
    }
  };
  auto barrier = [] {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };
  auto mfma16 = [](bf16x8 a, bf16x8 b, f32x4 c) {
    if constexpr (KNN)
      return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    else
      return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  };

  // prologue: K-tile 0 -> E, K-tile 1 -> O of the first tile
  bias_dma(t, 0);
  gS(sbase(t), 0, 0);
  gS(sbase(t), 1, 1);
  {
    const auto xb = xbase(t);
    const auto wb = wbase(t);
#pragma unroll
    for (int j = 0; j < 4; ++j) gA(xb, 0, j, 0);
#pragma unroll
    for (int j = 0; j < NT; ++j) gB(wb, 0, j, 0);
#pragma unroll
    for (int j = 0; j < 4; ++j) gA(xb, 1, j, 1);
#pragma unroll
    for (int j = 0; j < NT; ++j) gB(wb, 1, j, 1);
  }
  __builtin_amdgcn_s_waitcnt(vmcnt_n(4 + NT));
  barrier();
  if (wr == 1) barrier();  // stagger: m-group 1 runs one barrier behind

  bool first = true;
  int par = 0;
#ifdef MMR_P8_STAMPS
  unsigned long long* lst = (unsigned long long*)((char*)dsm + C::LDS_B - C::STAMP_B);
  int tcount = 0;
  auto stamp = [&](int k) {
    const unsigned long long v = k == 3 ? __builtin_amdgcn_s_memrealtime() : __builtin_amdgcn_s_memtime();
    if (lane == 0 && tcount < 8) lst[(wave * 8 + tcount) * 4 + k] = v;
  };
#else
  auto stamp = [](int) {};
#endif
  uint32_t sca[2] = {0u, 0u}, scb = 0u;  // FP8: this K-tile's E8M0 scales (m-tile i: byte i of sca; n-tile j: byte j of scb)
  while (true) {
    const int tnext = t + per;
    const bool has_next = tnext < hi;
    const auto xc = xbase(t);
    const auto wcb = wbase(t);
    const auto xn = xbase(has_next ? tnext : t);
    const auto wn = wbase(has_next ? tnext : t);
    const int n0 = nof(t) * TBN;
    const int64_t m0 = (int64_t)mof(t) * 256;
    const int sbc = sbase(t), sbn = sbase(has_next ? tnext : t);
    stamp(3);
    stamp(0);

    f32x4 acc[8][NT];
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // the residual (early_res): round rd, chunk c = the 16-B output chunk idx = 64 c + lane of the
    // epilogue's store pass (row idx / 2NT of the round's 16 RM rows, columns 8 (idx % 2NT) ..)
    uint4 rr16[early_res ? 8 / C::RM : 1][early_res ? C::CPL : 1];
    if constexpr (early_res) {
#pragma unroll
      for (int rd = 0; rd < 8 / C::RM; ++rd)
#pragma unroll
        for (int c = 0; c < C::CPL; ++c) {
          const int idx = c * 64 + lane;
          rr16[rd][c] = *(const uint4*)(R + (m0 + wr * 128 + rd * 16 * C::RM + idx / (2 * NT)) * N + n0 + wc * 16 * NT +
                                        (idx % (2 * NT)) * 8);
        }
    }

    for (int it = 0; it < nk / 2; ++it) {
      const bool last_it = it + 1 == nk / 2;
      const bool loads = !last_it || has_next;  // this iteration stages two more K-tiles
      const auto xl = last_it ? xn : xc;  // their tile: this one, or the next at the end
      const auto wl = last_it ? wn : wcb;
      const int ke = last_it ? 0 : 2 * it + 2, ko = ke + 1;
#pragma unroll
      for (int p = 0; p < 8; ++p) {
        const int buf = p >> 2, q = p & 3;
        // ---- load segment (s = 2p)
        if (q == 0) {
          if constexpr (FP8) {
            // native vector types on purpose: a HIP uint2 (struct) LDS read carries no TBAA, and hipcc
            // then waits vmcnt(0) for every in-flight LDS-DMA before it (drained the K-tile prefetch
            // at every K-tile: fp8 phases ran ~30 % longer than bf16's)
            typedef uint32_t u32x1_t __attribute__((ext_vector_type(1)));
            // lane offsets from a freshly computed lane id (opaque to hipcc): kept live across the
            // K loop they were spilled, and a spill reload is a vmcnt op that drains the prefetch
            int ll;
            asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ll));
            const uint8_t* sb = (const uint8_t*)(dsm + soff(buf));
            const u32x2 sa2 = *(const u32x2*)(sb + wr * 512 + ll * 8);  // ((wr 4 + fq) 16 + fr) 8
            sca[0] = sa2[0];
            sca[1] = sa2[1];
            scb = (*(const u32x1_t*)(sb + 1024 + wc * 256 + ll * 4))[0];
          }
#pragma unroll
          for (int i = 0; i < 4; ++i) ldA(buf, i, i);
#pragma unroll
          for (int j = 0; j < NH0; ++j) ldB0(buf, j);
        } else if (q == 1) {
#pragma unroll
          for (int j = 0; j < NT - NH0; ++j) ldB1(buf, j);
        } else if (q == 2) {
#pragma unroll
          for (int i = 0; i < 4; ++i) ldA(buf, i, 4 + i);
        }
        auto issue = [&](int sg) {
#ifdef MMR_P8_NOLOAD
          if (!KNN && !last_it) return;  // diagnostic build only: the K loop on stale LDS (results wrong)
#endif
          if (loads) {
            if (sg == 2) gA(xl, 0, 0, ke);
            if (sg == 3) { gS(last_it ? sbn : sbc, 0, ke); gA(xl, 0, 2, ke); }
            if (sg == 5) gB(wl, 0, 0, ke);
            if (sg == 6) { gB(wl, 0, 1, ke); gA(xl, 0, 1, ke); }
            if (sg == 7) { gB(wl, 0, 2, ke); gA(xl, 0, 3, ke); }
            if (sg == 8 && NT == 4) gB(wl, 0, 3, ke);
            if (sg == 10) gA(xl, 1, 0, ko);
            if (sg == 11) { gS(last_it ? sbn : sbc, 1, ko); gA(xl, 1, 2, ko); }
            if (sg == 13) gB(wl, 1, 0, ko);
            if (sg == 14) { gB(wl, 1, 1, ko); gA(xl, 1, 1, ko); }
            if (sg == 15) { gB(wl, 1, 2, ko); gA(xl, 1, 3, ko); if (NT == 4) gB(wl, 1, 3, ko); }
          }
        };
        issue(2 * p);
        if (p == 3) {  // end of s6: O complete (younger: E pieces, + last tile's stores at it 0)
          if (!loads) __builtin_amdgcn_s_waitcnt(vmcnt_n(0));
          else if (it == 0 && !first) __builtin_amdgcn_s_waitcnt(vmcnt_n(5 + nstore + NRES));
          else if (it == 0) __builtin_amdgcn_s_waitcnt(vmcnt_n(5 + NRES));
          else __builtin_amdgcn_s_waitcnt(vmcnt_n(5));
        } else if (p == 7) {  // end of s14: E complete (younger: 5 O pieces)
          if (loads) __builtin_amdgcn_s_waitcnt(vmcnt_n(5));
          else __builtin_amdgcn_s_waitcnt(vmcnt_n(0));
        }
        barrier();
        // ---- MFMA segment (s = 2p + 1)
        __builtin_amdgcn_s_setprio(1);
        const int mb = q < 2 ? 0 : 4;
        if constexpr (FP8) {
          // one 16x16x128 MX MFMA per (m-tile, n-tile): W fragment (src0, its scale) x X fragment
          // (src1) -> C^T like the bf16 form; opsel picks the tile's scale byte
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            if (i == 1) issue(2 * p + 1);
            const int mi = mb + i;
            if (q == 0 || q == 3) {
#pragma unroll
              for (int j = 0; j < NH0; ++j)
                acc[mi][j] = mx_mfma(fb08[j], fa8[i], acc[mi][j], scb, j, sca[mi >> 2], mi & 3);
            } else {
#pragma unroll
              for (int j = 0; j < NT - NH0; ++j)
                acc[mi][NH0 + j] = mx_mfma(fb18[j], fa8[i], acc[mi][NH0 + j], scb, NH0 + j, sca[mi >> 2], mi & 3);
            }
          }
        } else if constexpr (X3P) {
          // hi.hi, then lo.hi (w_lo . x_hi), then hi.lo (w_hi . x_lo): product-outermost, so 4 NH MFMAs
          // separate two into the same accumulator
          // (MMR_X3_PRODUCTS: diagnostic builds only — 1 = hi.hi alone, 6 = every product twice; results wrong)
          constexpr int wk[6] = {0, 1, 0, 0, 1, 0}, xk[6] = {0, 0, 1, 0, 0, 1};  // k-step (0 hi, 1 lo) of W / X
          constexpr int NPR = MMR_X3_PRODUCTS;
          if (q == 0 || q == 3) {
#pragma unroll
            for (int pr = 0; pr < NPR; ++pr)
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                if (pr == 0 && i == 1) issue(2 * p + 1);
#pragma unroll
                for (int j = 0; j < NH0; ++j) acc[mb + i][j] = mfma16(fb0[j][wk[pr]], fa[i][xk[pr]], acc[mb + i][j]);
              }
          } else {
#pragma unroll
            for (int pr = 0; pr < NPR; ++pr)
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                if (pr == 0 && i == 1) issue(2 * p + 1);
#pragma unroll
                for (int j = 0; j < NT - NH0; ++j)
                  acc[mb + i][NH0 + j] = mfma16(fb1[j][wk[pr]], fa[i][xk[pr]], acc[mb + i][NH0 + j]);
              }
          }
        } else if (q == 0 || q == 3) {
#pragma unroll
          for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              if (ks == 0 && i == 1) issue(2 * p + 1);
#pragma unroll
              for (int j = 0; j < NH0; ++j)
                acc[mb + i][j] = mfma16(fb0[j][ks], fa[i][ks], acc[mb + i][j]);
            }
        } else {
#pragma unroll
          for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              if (ks == 0 && i == 1) issue(2 * p + 1);
#pragma unroll
              for (int j = 0; j < NT - NH0; ++j)
                acc[mb + i][NH0 + j] = mfma16(fb1[j][ks], fa[i][ks], acc[mb + i][NH0 + j]);
            }
        }
        // FP8: the cluster's results are pinned before the barrier — machine sinking otherwise moves
        // the scaled MFMAs into later blocks (toward their next use) and keeps several phases of
        // fragments live (256 VGPRs + spills)
        if constexpr (FP8) {
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j)
              if ((q == 0 || q == 3) == (j < NH0)) mmr::pin(acc[mb + i][j]);
        }
        __builtin_amdgcn_s_setprio(0);
        barrier();
      }
    }

    stamp(1);
    // ---- epilogue (per wave, no workgroup barrier): C^T tiles (operands swapped) — lane has row
    // 16i + fr, columns 16j + 4fq + 0..3 — act(acc + bias) (+ residual) in f32 -> bf16 in the wave's
    // LDS area, RM m-tiles at a time -> 16-B row chunks -> Y
    // lane-derived addresses recomputed here from an opaque copy of the lane id, so hipcc does not
    // keep them live (and spilled) across the main loop
    int le = lane;
    asm volatile("" : "+v"(le));
    const int efr = le & 15, efq = le >> 4;
    if constexpr (KNN) {
      // lane: query m0 + wr 128 + 16 i + efr; gallery rows rj .. rj + 3 (rj = n0 + wc 64 + 16 j +
      // 4 efq) = the 2-row units rj / 2 and rj / 2 + 1 (one 8-B store); the wave column's 64 rows =
      // one block.  Every store issued (NSTORE exact for the next tile's counted wait)
      const int64_t r0 = n0 + wc * 64;
      // RS (raw-row galleries, the native fp16 index): the per-row 1 / |g| turning q^ . g into the cosine,
      // staged into LDS by LDS-DMA with the tile (bias_dma) — a global load here would retire behind the
      // next tile's K-tile prefetch and drain it
      f32x4 rs[4];
      if (RS) {
#pragma unroll
        for (int j = 0; j < 4; ++j) rs[j] = *(const f32x4*)(lbias + par * NV * TBN + wc * 64 + 16 * j + 4 * efq);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) rs[j] = (f32x4){1.f, 1.f, 1.f, 1.f};
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int64_t q = m0 + wr * 128 + i * 16 + efr;
        float bmx = -INFINITY;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int64_t rj = r0 + 16 * j + 4 * efq;
          float a[4];
#pragma unroll
          for (int rg = 0; rg < 4; ++rg) a[rg] = rj + rg < nval ? acc[i][j][rg] * rs[j][rg] : -INFINITY;
          const float2 u2 = make_float2(fmaxf(a[0], a[1]), fmaxf(a[2], a[3]));
          if constexpr (skip_gm) {
            asm volatile("" ::"v"(u2.x), "v"(u2.y));
          } else if constexpr (KNN == 2) {
            *(float2*)(GM + q * ldG + rj / 2) = u2;
          } else {
            GM[q * ldG + rj / 4] = fmaxf(u2.x, u2.y);
          }
          bmx = fmaxf(bmx, fmaxf(u2.x, u2.y));
        }
        bmx = fmaxf(bmx, __shfl_xor(bmx, 16, 64));
        bmx = fmaxf(bmx, __shfl_xor(bmx, 32, 64));
        if (efq == 0) BM[q * ldB + r0 / 64] = bmx;
      }
      if (!has_next) break;
      par ^= 1;
      bias_dma(tnext, par);
      t = tnext;
      first = false;
      continue;
    }
    f32x4 bq[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j)
      bq[j] = HAS_BIAS ? *(const f32x4*)(lbias + par * NV * TBN + wc * 16 * NT + j * 16 + efq * 4) : (f32x4){0.f, 0.f, 0.f, 0.f};
    // LNM: the column vectors of this lane's columns and the row coefficients of its 8 rows (LDS)
    auto lvec = [&](int v, int j) { return *(const f32x4*)(lbias + (par * NV + v) * TBN + wc * 16 * NT + j * 16 + efq * 4); };
    float ra[LNM ? 8 : 1], rb[LNM ? 8 : 1];  // LN(y) = ra y + rb per row (rstd, -mean rstd)
    if constexpr (LNM != 0) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float2 cf = *(const float2*)(lcoef + par * 512 + (wr * 128 + i * 16 + efr) * 2);
        ra[i] = cf.x;
        rb[i] = cf.y;
      }
    }
    if constexpr (OF32 && NT == 3) {
      // f32 output of the x3 split GEMM (NT = 3, every BERT / Swin / fusion x3 shape): staged per m-tile round
      // through the m-group's LDS epilogue area so the stores are row-major — the group's 4 waves (one per
      // n-column block of 48) write their 16 x 48 fragment values, one barrier, then wave wc stores rows
      // 4 wc .. 4 wc + 3 of the round's 16 rows across the tile's 192 columns: an instruction covers ~1.3
      // rows x 768 B of whole 128-B lines, where the fragment-layout stores (16 rows x 64 B per instruction)
      // ran the store phase at a quarter of the write path and held up the next tile's first waits (vmcnt is
      // in order): QKV 310 -> 159 us with no stores at all (profiles/r06_x3_epilogue_ab.txt).
      // OSPL stages the hi and lo bf16 images the same way and stores 16-B chunks of either.  Two barriers per
      // round (every wave runs the same 16); values and rounding exactly as the fragment-layout path.
      constexpr int RS = 16 * NT * 4 + 4;       // f32 row stride of the group's staging image (196)
      constexpr int RSH = 16 * NT * 4 + 8;      // bf16 row stride of an OSPL image (200)
      static_assert(!OSPL ? 16 * RS * 4 <= 4 * 16 * C::RM * C::ELD * 2 : 2 * 16 * RSH * 2 <= 4 * 16 * C::RM * C::ELD * 2,
                    "group staging image fits the group's epilogue areas");
      float* grp = (float*)(dsm + 2 * BUF + (wr * 4) * 16 * C::RM * C::ELD);
      uint16_t* grh = (uint16_t*)grp;          // OSPL: hi image [16][RSH], lo image behind it
      uint16_t* grl = grh + 16 * RSH;
      const int64_t tb = m0 * ldn * 4;
      const uint32_t nrec = (uint32_t)(256 * ldn * 4);
      const auto ry = __builtin_amdgcn_make_buffer_rsrc((void*)((char*)Y + tb), 0, (int)nrec, 0x00020000);
      const auto rr = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)R + (HAS_RES ? tb : 0)), 0, (int)nrec,
                                                        0x00020000);
#pragma unroll
      for (int i = 0; i < 8; ++i) {  // (unrolled: acc[i] must be a register, not an indexed array)
        // (1) fragment layout -> the group image: bias, erf GELU (A-S erf, |err| <= 1.5e-7), OSPL's split
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          f32x4 v = acc[i][j] + bq[j];
          if constexpr (ACT == 1) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = mmr::gelu_erf(v[e]);
          }
          const int cc = wc * 16 * NT + j * 16 + efq * 4;  // column in the tile
          if constexpr (OSPL) {
            // v pinned as the rounded f32 value: hipcc otherwise contracts the GELU's last multiply into
            // v - hi (an fma), and lo would no longer be the split of the f32 output
            mmr::pin(v);
            const uint32_t h0 = mmr::pack2bf(v[0], v[1]), h1 = mmr::pack2bf(v[2], v[3]);
            const uint32_t l0 = mmr::pack2bf(v[0] - __uint_as_float(h0 << 16), v[1] - __uint_as_float(h0 & 0xFFFF0000u));
            const uint32_t l1 = mmr::pack2bf(v[2] - __uint_as_float(h1 << 16), v[3] - __uint_as_float(h1 & 0xFFFF0000u));
            ds_write_b64_untracked(grh + efr * RSH + cc, h0, h1);
            ds_write_b64_untracked(grl + efr * RSH + cc, l0, l1);
          } else {
            ds_write_b128_untracked(grp + efr * RS + cc, __builtin_bit_cast(uint4, v));
          }
        }
        __builtin_amdgcn_s_waitcnt(LGKM0);  // lgkmcnt(0)
        barrier();
        // (2) rows 4 wc .. 4 wc + 3 of the round, row-major 16-B chunks (3 per lane)
        if constexpr (OSPL) {
          // 4 rows x (24 hi + 24 lo) chunks of 8 bf16
          uint4 ch[3];
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const int idx = c * 64 + le, part = idx / 96, k = idx % 96, r = k / 24, q = k % 24;
            ch[c] = *(const uint4*)((part ? grl : grh) + (4 * wc + r) * RSH + 8 * q);
          }
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const int idx = c * 64 + le, part = idx / 96, k = idx % 96, r = k / 24, q = k % 24;
            uint16_t* ys = Y + (m0 + wr * 128 + i * 16 + 4 * wc + r) * 2 * (int64_t)N + (part ? N : 0) + n0 + 8 * q;
            if (!skip_st) st16(ys, ch[c], false);
            else asm volatile("" ::"v"(ch[c].x), "v"(ch[c].y), "v"(ch[c].z), "v"(ch[c].w));
          }
        } else {
          f32x4 ov[3], rv[3];
          uint32_t off[3];
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const int idx = c * 64 + le, r = idx / (16 * NT), q = idx % (16 * NT);  // 48 f32x4 chunks per row
            const int rl = wr * 128 + i * 16 + 4 * wc + r, col = n0 + 4 * q;
            off[c] = col < ldn ? (uint32_t)((rl * ldn + col) * 4) : 0x7FFFFFF0u;
            if constexpr (HAS_RES) rv[c] = __builtin_amdgcn_raw_buffer_load_b128(rr, off[c], 0, 0);
            ov[c] = *(const f32x4*)(grp + (4 * wc + r) * RS + 4 * q);
          }
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            if constexpr (HAS_RES) ov[c] += rv[c];
            if (!skip_st) __builtin_amdgcn_raw_buffer_store_b128(ov[c], ry, off[c], 0, 0);
            else asm volatile("" ::"v"(ov[c]));
          }
        }
        __builtin_amdgcn_s_waitcnt(LGKM0);  // the image is read before the next round overwrites it
        barrier();
      }
    } else if constexpr (OF32) {
      // f32 output (the x3 towers' K' = 3K split GEMM): lane row 16 i + efr, columns 16 j + 4 efq .. + 3
      // -> one 16-B store per (i, j), no LDS round; bias, erf GELU (A-S erf, |err| <= 1.5e-7), then the f32 residual
      // (loaded per m-tile: they retire behind the next tile's prefetch, once per tile)
      // Y / R are [M][ldn] f32 with ldn <= N (N = the weight image's rows, padded to whole tiles): the
      // tile's 256 rows as one buffer (64-bit base in SGPRs, 32-bit offsets), columns >= ldn get an
      // offset past num_records — the store is dropped and the load returns 0 by the buffer range check,
      // while the instruction still issues, so the next tile's counted wait stays exact
      const int64_t tb = m0 * ldn * 4;
      const uint32_t nrec = (uint32_t)(256 * ldn * 4);
      const auto ry = __builtin_amdgcn_make_buffer_rsrc((void*)((char*)Y + tb), 0, (int)nrec, 0x00020000);
      const auto rr = __builtin_amdgcn_make_buffer_rsrc((void*)((const char*)R + (HAS_RES ? tb : 0)), 0, (int)nrec,
                                                        0x00020000);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int rl = wr * 128 + i * 16 + efr;  // row in the tile
        uint32_t off[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          const int col = n0 + wc * 16 * NT + j * 16 + efq * 4;
          off[j] = col < ldn ? (uint32_t)((rl * ldn + col) * 4) : 0x7FFFFFF0u;
        }
        f32x4 rr4[HAS_RES ? NT : 1];
        if constexpr (HAS_RES) {
#pragma unroll
          for (int j = 0; j < NT; ++j) rr4[j] = __builtin_amdgcn_raw_buffer_load_b128(rr, off[j], 0, 0);
        }
        uint2 ph[OSPL ? NT : 1], pl[OSPL ? NT : 1];  // OSPL: the hi / lo bf16 quads of each n-tile
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          f32x4 v = acc[i][j] + bq[j];
          if constexpr (ACT == 1) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = mmr::gelu_erf(v[e]);  // A-S erf (1.5e-7): x3 mode, as linear_x3
          }
          if constexpr (HAS_RES) v += rr4[j];
          if constexpr (OSPL) {
            // [hi | lo] bf16 of the f32 value (the split mmr_x3_split_rows would make), row width 2 N; v pinned
            // as the rounded f32 value: hipcc otherwise contracts the GELU's last multiply into v - hi (an fma),
            // and lo would no longer be the split of the f32 output (bitwise tests against the f32 route)
            mmr::pin(v);
            const uint32_t h0 = mmr::pack2bf(v[0], v[1]), h1 = mmr::pack2bf(v[2], v[3]);
            ph[j] = make_uint2(h0, h1);
            pl[j] = make_uint2(mmr::pack2bf(v[0] - __uint_as_float(h0 << 16), v[1] - __uint_as_float(h0 & 0xFFFF0000u)),
                               mmr::pack2bf(v[2] - __uint_as_float(h1 << 16), v[3] - __uint_as_float(h1 & 0xFFFF0000u)));
          } else if (!skip_st) {
            __builtin_amdgcn_raw_buffer_store_b128(v, ry, off[j], 0, X3ST_AUX);
          }
        }
        if constexpr (OSPL) {
          // n-tile pairs (j, j + 1) through v_permlane16_swap as the GELU epilogue does (epi_pl): every lane
          // then holds 8 consecutive columns, so hi and lo go out as one 16-B store each per pair — a row's
          // 4 lanes write the pair's 64 contiguous bytes (8-B stores per tile wrote 32-B segments, twice the
          // instructions); an odd last tile pairs with itself (lanes fq 0 / 1 and 2 / 3 write the same bytes)
#pragma unroll
          for (int j = 0; j < NT; j += 2) {
            const int j2 = j + 1 < NT ? j + 1 : j;
            const auto hx = __builtin_amdgcn_permlane16_swap(ph[j].x, ph[j2].x, false, false);
            const auto hy = __builtin_amdgcn_permlane16_swap(ph[j].y, ph[j2].y, false, false);
            const auto lx = __builtin_amdgcn_permlane16_swap(pl[j].x, pl[j2].x, false, false);
            const auto ly = __builtin_amdgcn_permlane16_swap(pl[j].y, pl[j2].y, false, false);
            const int col = n0 + wc * 16 * NT + 16 * j + (j2 != j && (efq & 1) ? 16 : 0) + (efq >> 1) * 8;
            uint16_t* ys = Y + (m0 + rl) * 2 * (int64_t)N + col;
            if (!skip_st) {
              st16(ys, make_uint4(hx[0], hy[0], hx[1], hy[1]), X3ST_AUX != 0);
              st16(ys + N, make_uint4(lx[0], ly[0], lx[1], ly[1]), X3ST_AUX != 0);
            } else {
              asm volatile("" ::"v"(hx[0]), "v"(hy[0]), "v"(lx[0]), "v"(ly[0]));
            }
          }
        }
      }
    }
    uint2 rq[HAS_RES && !early_res ? 8 : 1][HAS_RES && !early_res ? NT : 1];  // (unused by OF32)
    if constexpr (HAS_RES && !early_res && !OF32) {
#pragma unroll
      for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
          rq[i][j] = *(const uint2*)(R + (m0 + wr * 128 + i * 16 + efr) * N + n0 + wc * 16 * NT + j * 16 + efq * 4);
    }
    f32x4 cqr[LNM == 1 && epi_pl ? NT : 1];  // the fold vector of the lane's columns, held for the GELU epilogue
    if constexpr (LNM == 1 && epi_pl) {
#pragma unroll
      for (int j = 0; j < NT; ++j) cqr[j] = lvec(1, j);
    }
    if constexpr (epi_pl) {
      // C^T fragment -> 16-B row chunks in registers: for an n-tile pair (j, j + 1) one
      // v_permlane16_swap per dword hands lane group fq = 1 (3) the pair's tile-(j+1) columns
      // 0-3 (8-11) of fq = 0 (2) and takes back tile j's columns 4-7 (12-15), so every lane holds
      // 8 consecutive columns of its row: fq 0 -> tile j cols 0-7, fq 1 -> tile j+1 cols 0-7,
      // fq 2 -> tile j cols 8-15, fq 3 -> tile j+1 cols 8-15 (an odd last tile pairs with itself:
      // lanes fq 0/1 and 2/3 then write the same bytes).  One dwordx4 store per pair and m-tile.
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int64_t row = m0 + wr * 128 + i * 16 + efr;
#pragma unroll
        for (int j = 0; j < NT; j += 2) {
          const int j2 = j + 1 < NT ? j + 1 : j;
          uint2 pk[2];
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int jj = h ? j2 : j;
            float v[4];
#pragma unroll
            for (int rg = 0; rg < 4; rg += 2) {
              mmr::f32x2_t u;
              if constexpr (LNM == 1)
                u = (mmr::f32x2_t){fmaf(ra[i], acc[i][jj][rg], fmaf(rb[i], cqr[jj][rg], bq[jj][rg])),
                                   fmaf(ra[i], acc[i][jj][rg + 1], fmaf(rb[i], cqr[jj][rg + 1], bq[jj][rg + 1]))};
              else
                u = (mmr::f32x2_t){acc[i][jj][rg] + bq[jj][rg], acc[i][jj][rg + 1] + bq[jj][rg + 1]};
              if (ACT == 1) u = mmr::gelu_fast2(u);
              v[rg] = u.x;
              v[rg + 1] = u.y;
            }
            if constexpr (HAS_RES) {
              const uint2 rv = rq[i][jj];
              v[0] += __uint_as_float(rv.x << 16);
              v[1] += __uint_as_float(rv.x & 0xFFFF0000u);
              v[2] += __uint_as_float(rv.y << 16);
              v[3] += __uint_as_float(rv.y & 0xFFFF0000u);
            }
            pk[h] = make_uint2(mmr::pack2bf(v[0], v[1]), mmr::pack2bf(v[2], v[3]));
          }
          const auto sx = __builtin_amdgcn_permlane16_swap(pk[0].x, pk[1].x, false, false);
          const auto sy = __builtin_amdgcn_permlane16_swap(pk[0].y, pk[1].y, false, false);
          const int col = n0 + wc * 16 * NT + 16 * j + (j2 != j && (efq & 1) ? 16 : 0) + (efq >> 1) * 8;
          if (!skip_st) st16(Y + row * N + col, make_uint4(sx[0], sy[0], sx[1], sy[1]), false);
          else asm volatile("" ::"v"(sx[0]), "v"(sy[0]), "v"(sx[1]), "v"(sy[1]));
        }
      }
    }
#pragma unroll
    for (int rd = 0; rd < ((epi_pl || OF32) ? 0 : 8 / C::RM); ++rd) {  // LDS-staged rounds
      if constexpr (early_res) {  // the round's residual chunks -> the wave's LDS area (row layout)
#pragma unroll
        for (int c = 0; c < C::CPL; ++c) {
          const int idx = c * 64 + le;
          ds_write_b128_untracked(et + (idx / (2 * NT)) * C::ELD + (idx % (2 * NT)) * 8, rr16[rd][c]);
        }
        __builtin_amdgcn_s_waitcnt(LGKM0);  // lgkmcnt(0)
        __builtin_amdgcn_wave_barrier();
      }
#pragma unroll
      for (int ii = 0; ii < C::RM; ++ii) {
        const int i = rd * C::RM + ii;
        float st1 = 0.f;     // STO: this row's sum over the lane's columns
        uint32_t sw[STO ? 2 * NT : 1];  // STO: the lane's stored (bf16-rounded) outputs, for the centred pass
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          float v[4];
          f32x4 cq;
          if constexpr (LNM == 1) cq = lvec(1, j);
#pragma unroll
          for (int rg = 0; rg < 4; rg += 2) {
            mmr::f32x2_t u;
            if constexpr (LNM == 1)
              u = (mmr::f32x2_t){fmaf(ra[i], acc[i][j][rg], fmaf(rb[i], cq[rg], bq[j][rg])),
                                 fmaf(ra[i], acc[i][j][rg + 1], fmaf(rb[i], cq[rg + 1], bq[j][rg + 1]))};
            else
              u = (mmr::f32x2_t){acc[i][j][rg] + bq[j][rg], acc[i][j][rg + 1] + bq[j][rg + 1]};
            if (ACT == 1) u = OUT8 ? mmr::gelu_q8x2(u) : mmr::gelu_fast2(u);  // e4m3 output: the cheap form
            v[rg] = u.x;
            v[rg + 1] = u.y;
          }
          if constexpr (HAS_RES) {
            // early_res: read back in the fragment layout from the very 8 bytes this lane overwrites
            // with its output below (lane-private: no barrier between the read and the write)
            const uint2 rv = early_res ? *(const uint2*)(et + (ii * 16 + efr) * C::ELD + j * 16 + efq * 4) : rq[i][j];
            float r4[4] = {__uint_as_float(rv.x << 16), __uint_as_float(rv.x & 0xFFFF0000u),
                           __uint_as_float(rv.y << 16), __uint_as_float(rv.y & 0xFFFF0000u)};
            if constexpr (LNM == 2) {
              const f32x4 g = lvec(1, j), be = lvec(2, j);
#pragma unroll
              for (int e = 0; e < 4; ++e) r4[e] = fmaf(g[e], fmaf(ra[i], r4[e], rb[i]), be[e]);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] += r4[e];
          }
          const uint32_t p0 = mmr::pack2bf(v[0], v[1]), p1 = mmr::pack2bf(v[2], v[3]);
          if constexpr (STO) {
            const float w0 = __uint_as_float(p0 << 16), w1 = __uint_as_float(p0 & 0xFFFF0000u);
            const float w2 = __uint_as_float(p1 << 16), w3 = __uint_as_float(p1 & 0xFFFF0000u);
            st1 += (w0 + w1) + (w2 + w3);
            sw[2 * j] = p0;
            sw[2 * j + 1] = p1;
          }
          ds_write_b64_untracked(et + (ii * 16 + efr) * C::ELD + j * 16 + efq * 4, p0, p1);
        }
        if constexpr (STO) {
          // sum over the row's 4 lanes (fq): lane swaps on the VALU (no LDS round trip)
          auto sum4 = [](float v) {
            const auto p = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
            const float h = __uint_as_float(p[0]) + __uint_as_float(p[1]);
            const auto q = __builtin_amdgcn_permlane16_swap(__float_as_uint(h), __float_as_uint(h), false, false);
            return __uint_as_float(q[0]) + __uint_as_float(q[1]);
          };
          // the part's (sum, centred sum of squares M2) over its 16 NT columns — Chan's parallel form,
          // merged in mmr_ln_row_coef (a raw sum of squares loses the variance of rows whose |mean| is
          // large against their spread: ADVICE r04)
          st1 = sum4(st1);
          const float pm = st1 * (1.0f / (16 * NT));
          float st2 = 0.f;
#pragma unroll
          for (int q = 0; q < 2 * NT; ++q) {
            const float d0 = __uint_as_float(sw[q] << 16) - pm, d1 = __uint_as_float(sw[q] & 0xFFFF0000u) - pm;
            st2 = fmaf(d0, d0, fmaf(d1, d1, st2));
          }
          st2 = sum4(st2);
          if (efq == 0)
            *(float2*)(SP + ((m0 + wr * 128 + i * 16 + efr) * (int64_t)(4 * tiles_n) + nof(t) * 4 + wc) * 2) =
                make_float2(st1, st2);
        }
      }
      __builtin_amdgcn_s_waitcnt(LGKM0);  // lgkmcnt(0)
      __builtin_amdgcn_wave_barrier();
      if constexpr (OUT8) {
        // lane: row le/4 of the round's 16 rows, columns 16 (le % 4) .. +15 of the wave's 64
        const int rr = le >> 2, hb = le & 3;
        const bf16x8 h0 = *(const bf16x8*)(et + rr * C::ELD + (2 * hb) * 8);
        const bf16x8 h1 = *(const bf16x8*)(et + rr * C::ELD + (2 * hb + 1) * 8);
        float v[16];
        float amax = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          v[e] = mmr::bf2f((uint16_t)h0[e]);
          v[8 + e] = mmr::bf2f((uint16_t)h1[e]);
          amax = fmaxf(amax, fmaxf(fabsf(v[e]), fabsf(v[8 + e])));
        }
        amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
        const uint32_t ab = __float_as_uint(amax);
        int ex = (int)((ab >> 23) & 255) - 127 - 8 + ((ab & 0x7FFFFF) > 0x600000 ? 1 : 0);
        ex = ex < -127 ? -127 : (ex > 126 ? 126 : ex);
        const float inv = __uint_as_float((uint32_t)(127 - ex) << 23);
        uint32_t w4[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          w4[i] = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(v[4 * i] * inv, v[4 * i + 1] * inv, 0, false);
          w4[i] = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(v[4 * i + 2] * inv, v[4 * i + 3] * inv, (int)w4[i], true);
        }
        const int64_t m = m0 + wr * 128 + rd * 16 + rr;
        const int n = n0 + wc * 64 + hb * 16;
        st16((uint8_t*)Y + m * N + n, make_uint4(w4[0], w4[1], w4[2], w4[3]), (ntst & 1) != 0);
        if ((hb & 1) == 0) {  // one scale byte per 32-block, layout-0 image: [m/256][n/128][wr][fq][fr][i]
          const int fq = (n % 128) / 32;
          YS[((m0 / 256) * (N / 128) + n / 128) * 1024 + ((wr * 4 + fq) * 16 + rr) * 8 + rd] = (uint8_t)(ex + 127);
        }
      } else {
        bf16x8 ov[C::CPL];
#pragma unroll
        for (int c = 0; c < C::CPL; ++c) {
          const int idx = c * 64 + le;
          ov[c] = *(const bf16x8*)(et + (idx / (2 * NT)) * C::ELD + (idx % (2 * NT)) * 8);
        }
#pragma unroll
        for (int c = 0; c < C::CPL; ++c) {
          const int idx = c * 64 + le;
          const int64_t m = m0 + wr * 128 + rd * 16 * C::RM + idx / (2 * NT);
          const int n = n0 + wc * 16 * NT + (idx % (2 * NT)) * 8;
          if (!skip_st) st16(Y + m * N + n, __builtin_bit_cast(uint4, ov[c]), (ntst & 1) != 0);
          else asm volatile("" ::"v"(ov[c]));
        }
      }
      __builtin_amdgcn_s_waitcnt(LGKM0);
      __builtin_amdgcn_wave_barrier();
    }
    stamp(2);
#ifdef MMR_P8_STAMPS
    ++tcount;
#endif
    if (!has_next) break;
    par ^= 1;
    bias_dma(tnext, par);
    t = tnext;
    first = false;
  }
  if (wr == 0) barrier();  // balance the stagger
  __builtin_amdgcn_s_waitcnt(vmcnt_n(0));
#ifdef MMR_P8_STAMPS
  __builtin_amdgcn_s_waitcnt(LGKM0);
  __syncthreads();
  if (blockIdx.x < 1024 && tid < 8 * 8 * 4) p8_stamps[blockIdx.x * 256 + tid] = lst[tid];
#endif
#endif
}

// ---------------------------------------------------------------- 4-wave persistent large-tile GEMM
// One wave per SIMD with a 128 x 16NT wave tile (NT = 8: 256 x 256 workgroup tile; NT = 6:
// 256 x 192): twice the MFMA work per LDS fragment byte of the 8-wave 64x64 layout; the 8 x NT
// accumulators (<= 256 f32) live in AGPRs.  KB = 64, two LDS stages.
// Persistent: one workgroup per CU walks its XCD's share of the tiles (consecutive tiles, so the
// X row panel and W stay in that XCD's L2).  The last slice of a tile issues the glds of the NEXT
// tile's first slice, and the epilogue stages 16 rows at a time through a small per-wave LDS
// area outside the two stages, so the next tile's loads are in flight while this tile's bias /
// GELU / residual / 16-B row stores run; the next tile's first wait counts the stores out
// (vmcnt(NSTORE)) instead of draining them.
constexpr int EPI4_PAD = 8;

template <int NT>
constexpr size_t w4_lds_bytes() {
  return 2ull * (256 + 32 * NT) * 64 * 2 + 4ull * 16 * (16 * NT + EPI4_PAD) * 2 + 32ull * NT * 4;
}

template <int NT, int ACT, bool HAS_BIAS, bool HAS_RES>
__global__ __launch_bounds__(256) void gemm_bf16_tn_w4(const uint16_t* __restrict__ X,
                                                       const uint16_t* __restrict__ W,
                                                       const float* __restrict__ bias,
                                                       const uint16_t* __restrict__ R,
                                                       uint16_t* __restrict__ Y, int64_t M, int N,
                                                       int K, int tiles_m, int tiles_n) {
  constexpr int MT = 8, KB = 64, RPI = 8;
  constexpr int TBM = 256, TBN = 32 * NT;
  constexpr int TA = TBM * KB, TB = TBN * KB;  // bf16 elements per stage
  constexpr int PA = TBM / RPI / 4, PB = TBN / RPI / 4;  // glds pieces per wave per stage
  constexpr int ELD = 16 * NT + EPI4_PAD;
  constexpr int CPR = 2 * NT;            // 16-B chunks per wave-tile row
  constexpr int CPL = 16 * CPR / 64;     // chunks per lane per 16-row group
  constexpr int NSTORE = MT * CPL;       // global stores per wave per tile
  constexpr int NLOADS = 0;  // the bias tile travels by LDS-DMA with slice 0 (no registers in the loop)
  static_assert(NSTORE <= 63 && NLOADS <= 63, "vmcnt range");
  extern __shared__ __attribute__((aligned(16))) uint16_t dsm[];  // [2][TA + TB] + epilogue

  const int ntiles = tiles_m * tiles_n;
  const int per = gridDim.x / 8, xcd = blockIdx.x % 8, slot = blockIdx.x / 8;
  const int lo = (int)((int64_t)ntiles * xcd / 8), hi = (int)((int64_t)ntiles * (xcd + 1) / 8);
  int t = lo + slot;
  if (t >= hi) return;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 15, fq = lane >> 4;
  const int nk = K / KB;

  // glds sources: piece p of A covers rows RPI*(wave + 4p) .. +7, lane -> (row, swizzled chunk).
  // 32-bit element offsets from the uniform base (saddr form, one VGPR per piece); rows past M are
  // clamped to M-1 (their products are never stored); N % TBN == 0 and K % 64 == 0 (launcher).
  // Per-lane byte offsets inside a tile's row panels are tile-independent (one VGPR per piece,
  // glds in saddr form); a tile contributes only uniform bases.  The last row tile is shifted up
  // to end at row M (M >= 256): its first rows recompute rows of the previous tile, and writing
  // those identical values twice is harmless — no per-row clamping or zero page in the loop.
  const int prow_in = lane >> 3, pch = lane & 7;
  uint32_t offA[PA], offB[PB];
#pragma unroll
  for (int j = 0; j < PA; ++j) {
    const int row = RPI * (wave + 4 * j) + prow_in;
    offA[j] = (uint32_t)((row * K + swz(row, pch) * 8) * 2);
  }
#pragma unroll
  for (int j = 0; j < PB; ++j) {
    const int row = RPI * (wave + 4 * j) + prow_in;
    offB[j] = (uint32_t)((row * K + swz(row, pch) * 8) * 2);
  }
  const char* Xt = nullptr;  // this tile's panels (uniform)
  const char* Wt = nullptr;
  uint32_t kofs = 0;         // byte offset of the next slice to load
  auto tile_m0 = [&](int tile) { return std::min<int64_t>((int64_t)(tile / tiles_n) * TBM, M - TBM); };
  auto setup = [&](int tile) {
    Xt = (const char*)(X + tile_m0(tile) * K);
    Wt = (const char*)(W + (int64_t)(tile % tiles_n) * TBN * K);
    kofs = 0;
  };
  auto piece = [&](int s, int p, uint32_t ko) {
    uint16_t* la = dsm + s * (TA + TB);
    if (p < PA)
      __builtin_amdgcn_global_load_lds((const void*)(Xt + (offA[p] + ko)), (lds_ptr_t)(la + RPI * (wave + 4 * p) * KB), 16, 0, 0);
    else
      __builtin_amdgcn_global_load_lds((const void*)(Wt + (offB[p - PA] + ko)), (lds_ptr_t)(la + TA + RPI * (wave + 4 * (p - PA)) * KB), 16, 0, 0);
  };

  setup(t);
#pragma unroll
  for (int p = 0; p < PA + PB; ++p) piece(0, p, 0);
  kofs = KB * 2;
  int sb = 0;            // stage holding the slice about to be consumed
  bool stores_out = false;  // previous tile's epilogue stores may still be in flight
  uint16_t* et = dsm + 2 * (TA + TB) + wave * 16 * ELD;
  float* lbias = (float*)(dsm + 2 * (TA + TB) + 4 * 16 * ELD);  // [TBN] f32

  while (true) {
    const int64_t m0 = tile_m0(t);
    const int n0 = (t % tiles_n) * TBN;
    const int tnext = t + per;
    const bool has_next = tnext < hi;

    f32x4 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // the bias tile (TBN floats) lands in LDS by one LDS-DMA issued with slice 0, so no bias
    // registers live across the main loop; the residual (accumulator layout) is fetched whole at
    // the start of the epilogue
    uint2 rq[HAS_RES ? MT : 1][HAS_RES ? NT : 1];
    for (int kt = 0; kt < nk; ++kt) {
      // glds of this slice were issued before: the previous tile's stores (kt = 0) or this tile's
      // epilogue operands (kt = 1) may stay in flight
      if (kt == 0 && stores_out) __builtin_amdgcn_s_waitcnt(vmcnt_n(NSTORE));
      else if (kt == 1) __builtin_amdgcn_s_waitcnt(vmcnt_n(NLOADS));
      else __builtin_amdgcn_s_waitcnt(vmcnt_n(0));
      asm volatile("" ::: "memory");
      __builtin_amdgcn_s_barrier();  // slice landed for every wave; the other stage is free
      asm volatile("" ::: "memory");
      if (HAS_BIAS && kt == 0 && wave == 0 && lane < TBN / 4)  // previous epilogue is past the barrier
        __builtin_amdgcn_global_load_lds((const void*)(bias + n0 + lane * 4), (lds_ptr_t)lbias, 16, 0, 0);
      const bool last = kt + 1 == nk;
      if (last && has_next) setup(tnext);  // the last slice prefetches the next tile's first
      // after the very last slice the loads are issued anyway (branch-free), re-reading slice 0
      const uint32_t ko = (last && !has_next) ? 0u : kofs;
      const int s = sb;
      const uint16_t* la = dsm + s * (TA + TB);
      const uint16_t* lb = la + TA;
      auto rdA = [&](int ks, int i) {
        const int rowa = wm * 128 + i * 16 + fr;
        return *(const bf16x8*)(la + rowa * KB + swz(rowa, ks * 4 + fq) * 8);
      };
      auto rdB = [&](int ks, int j) {
        const int rowb = wn * 16 * NT + j * 16 + fr;
        return *(const bf16x8*)(lb + rowb * KB + swz(rowb, ks * 4 + fq) * 8);
      };
      bf16x8 a0[MT], b0[NT], a1[MT], b1[NT];
#pragma unroll
      for (int j = 0; j < NT; ++j) b0[j] = rdB(0, j);
#pragma unroll
      for (int i = 0; i < MT; ++i) a0[i] = rdA(0, i);
      // k-step 0: per A row-tile i, the next slice's glds pieces (source order is kept: glds are
      // scheduling barriers for hipcc) and one k-step-1 fragment, then NT MFMAs
#pragma unroll
      for (int i = 0; i < MT; ++i) {
#pragma unroll
        for (int p = i * (PA + PB) / MT; p < (i + 1) * (PA + PB) / MT; ++p) piece(s ^ 1, p, ko);
        a1[i] = rdA(1, i);
        if (i < NT) b1[i] = rdB(1, i);
#pragma unroll
        for (int j = 0; j < NT; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b0[j], a0[i], acc[i][j], 0, 0, 0);
      }
      kofs += KB * 2;
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b1[j], a1[i], acc[i][j], 0, 0, 0);
      sb ^= 1;
    }

    // epilogue, 16 rows at a time: act(acc + bias) (+ residual) in f32 -> bf16 in the wave's LDS
    // area -> 16-B row chunks -> Y
    if constexpr (HAS_RES) {
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
          rq[i][j] = *(const uint2*)(R + (m0 + wm * 128 + i * 16 + fr) * N + n0 + wn * 16 * NT + j * 16 + fq * 4);
    }
#pragma unroll
    for (int i = 0; i < MT; ++i) {
#pragma unroll
      for (int j = 0; j < NT; ++j) {
        float v[4];
        const f32x4 bq = HAS_BIAS ? *(const f32x4*)(lbias + wn * 16 * NT + j * 16 + fq * 4) : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
          v[rg] = acc[i][j][rg] + bq[rg];
          if (ACT == 1) v[rg] = mmr::gelu_fast(v[rg]);
        }
        if constexpr (HAS_RES) {
          const uint2 q = rq[i][j];
          v[0] += __uint_as_float(q.x << 16);
          v[1] += __uint_as_float(q.x & 0xFFFF0000u);
          v[2] += __uint_as_float(q.y << 16);
          v[3] += __uint_as_float(q.y & 0xFFFF0000u);
        }
        *(uint2*)(et + fr * ELD + j * 16 + fq * 4) = make_uint2(mmr::pack2bf(v[0], v[1]), mmr::pack2bf(v[2], v[3]));
      }
      __builtin_amdgcn_s_waitcnt(LGKM0);
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int c = 0; c < CPL; ++c) {
        const int idx = c * 64 + lane;
        const int64_t m = m0 + wm * 128 + i * 16 + idx / CPR;
        const int n = n0 + wn * 16 * NT + (idx % CPR) * 8;
        *(bf16x8*)(Y + m * N + n) = *(const bf16x8*)(et + (idx / CPR) * ELD + (idx % CPR) * 8);
      }
      __builtin_amdgcn_s_waitcnt(LGKM0);
      __builtin_amdgcn_wave_barrier();
    }
    if (!has_next) break;
    t = tnext;
    stores_out = true;
  }
  __builtin_amdgcn_s_waitcnt(vmcnt_n(0));  // no LDS-DMA may land after the workgroup retires
}

// ---------------------------------------------------------------- MX-fp8 quantizer
// bf16 [rows][k] -> OCP e4m3 bytes [rows][kp] (zero-padded to kp) + one E8M0 scale per 32 consecutive
// k of a row: scale 2^e with the smallest e such that amax <= 448 * 2^e (exact from amax's bits, no
// clipping), q = round-to-nearest-even(x * 2^-e) (v_cvt_pk_fp8_f32).  The scales are written in
// the order the GEMM's per-lane LDS scale image wants (1 KB per operand panel and 128-k K-tile):
//   LAYOUT 0 (X, panels of 256 rows): [panel][kt][wr 2][fq 4][fr 16][i 8], row = 128 wr + 16 i + fr
//   LAYOUT 1 (W, panels of 192 rows): [panel][kt][wc 4][fq 4][fr 16][j 4], row = 48 wc + 16 j + fr
// (fq = the 32-block within the K-tile).
template <int LAYOUT>
__global__ __launch_bounds__(256) void quantize_mxfp8(const uint16_t* __restrict__ x, int64_t rows, int k,
                                                      int kp, uint8_t* __restrict__ q, uint8_t* __restrict__ sc) {
  // one thread per 16 values (two 16-B bf16 loads, one 16-B fp8 store), 2 threads per 32-block
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int c16n = kp / 16;
  const int64_t row = t / c16n;
  const int k0 = (int)(t % c16n) * 16;
  const bool ok = row < rows;
  const int64_t rc = ok ? row : rows - 1;
  const int ka = k0 < k ? k0 : k - 8, kb = k0 + 8 < k ? k0 + 8 : k - 8;
  const bf16x8 r0 = *(const bf16x8*)(x + rc * k + ka);  // unconditional (clamped), masked below
  const bf16x8 r1 = *(const bf16x8*)(x + rc * k + kb);
  float v[16];
  float amax = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    v[e] = k0 < k ? mmr::bf2f((uint16_t)r0[e]) : 0.f;
    v[8 + e] = k0 + 8 < k ? mmr::bf2f((uint16_t)r1[e]) : 0.f;
    amax = fmaxf(amax, fmaxf(fabsf(v[e]), fabsf(v[8 + e])));
  }
  amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
  const uint32_t ab = __float_as_uint(amax);
  int ex = (int)((ab >> 23) & 255) - 127 - 8 + ((ab & 0x7FFFFF) > 0x600000 ? 1 : 0);
  ex = ex < -127 ? -127 : (ex > 126 ? 126 : ex);
  const float inv = __uint_as_float((uint32_t)(127 - ex) << 23);  // 2^-ex, exact
  uint32_t w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    w[i] = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(v[4 * i] * inv, v[4 * i + 1] * inv, 0, false);
    w[i] = (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(v[4 * i + 2] * inv, v[4 * i + 3] * inv, (int)w[i], true);
  }
  if (!ok) return;
  *(uint4*)(q + row * kp + k0) = make_uint4(w[0], w[1], w[2], w[3]);
  if ((k0 & 31) == 0) {
    const int blk = k0 / 32, kt = blk / 4, fq = blk % 4;
    int64_t off;
    if (LAYOUT == 0) {
      const int64_t P = row / 256;
      const int rr = (int)(row % 256), wr = rr / 128, i = (rr % 128) / 16, fr = rr % 16;
      off = (P * (kp / 128) + kt) * 1024 + ((wr * 4 + fq) * 16 + fr) * 8 + i;
    } else {  // weights: panels of 64 NT rows (NT = 3 for layout 1, 4 for layout 2)
      constexpr int PR = LAYOUT == 1 ? 192 : 256, WT = PR / 4;
      const int64_t P = row / PR;
      const int rr = (int)(row % PR), wc = rr / WT, j = (rr % WT) / 16, fr = rr % 16;
      off = (P * (kp / 128) + kt) * 1024 + ((wc * 4 + fq) * 16 + fr) * 4 + j;
    }
    sc[off] = (uint8_t)(ex + 127);
  }
}

// The 8-phase GEMM's arguments by name (host side; the kernel keeps its positional signature).  A launch
// site sets the groups its form of the kernel reads and leaves the rest at their defaults.
struct P8Args {
  // operands and shape: M a multiple of 256, N of the tile width 64 NT (FP8: byte matrices, K in bytes)
  const uint16_t* x = nullptr;
  const uint16_t* w = nullptr;
  const float* bias = nullptr;
  const uint16_t* r = nullptr;
  uint16_t* y = nullptr;
  int64_t m = 0;
  int n = 0, k = 0;
  // FP8 / OUT8: the MX-fp8 scale images of X and W, and of the output
  const uint8_t* xs = nullptr;
  const uint8_t* ws = nullptr;
  uint8_t* ys = nullptr;
  // KNN: unit and block maxima with their row strides, the valid gallery rows, inverse row norms
  float* gm = nullptr;
  float* bm = nullptr;
  int64_t ldg = 0, ldb = 0, nval = 0;
  const float* rs = nullptr;
  int ntst = 0;  // non-temporal output stores (p8_nt)
  // LNM / STO: row coefficients, the fold's column vectors, row statistics out
  const float* lc = nullptr;
  const float* v1 = nullptr;
  const float* v2 = nullptr;
  float* sp = nullptr;
  int ldn = 0;  // OF32: the output's row width (N is padded to the tile width)
};

// The one launch of gemm_bf16_tn_p8: persistent grid of a multiple of 8 workgroups (one per CU, tiles split
// evenly per XCD), at most the tile count rounded down to 8 and at least 8.
template <int NT, int ACT, bool HB, bool HR, bool FP8 = false, bool OUT8 = false, int KNN = 0, int LNM = 0,
          bool STO = false, bool OF32 = false, bool OSPL = false, bool X3P = false>
void launch_p8(const P8Args& a, hipStream_t st) {
  constexpr int NV = LNM == 2 ? 3 : (LNM == 1 ? 2 : 1);
  const int tm = (int)(a.m / 256), tn = a.n / (64 * NT);
  const int64_t cus = std::max(8, cu_count() / 8 * 8);
  const int64_t grid = std::max<int64_t>(8, std::min<int64_t>(cus, (int64_t)tm * tn) / 8 * 8);
  gemm_bf16_tn_p8<NT, ACT, HB, HR, FP8, OUT8, KNN, LNM, STO, OF32, OSPL, X3P>
      <<<dim3((unsigned)grid), dim3(512), P8<NT, FP8, 0, NV>::LDS_B, st>>>(
          a.x, a.w, a.bias, a.r, a.y, a.m, a.n, a.k, tm, tn, a.xs, a.ws, a.ys, a.gm, a.bm, a.ldg, a.ldb, a.nval,
          a.ntst, a.rs, a.lc, a.v1, a.v2, a.sp, a.ldn);
}

// Kernel variants: (w4, cfg) pairs the launcher understands.  w4: 0 no persistent kernel, 1 the
// 4-wave persistent kernel (256x256 or 256x192 tiles), 2 persistent 256x192 only; cfg: the 8-wave
// tile when w4 does not apply (0 off -> 128x128; 1 256x256 KB64 x2; 2 256x256 KB32 x4;
// 3 256x128 KB64 x3; 4 / 5 256x128 KB32 x2 / x3; 6 256x192 KB64 x2 — N = 768 / 2304 / 3072 at
// M = 32768 give 512 / 1536 / 2048 tiles, whole rounds of 256 CUs where 256x256 leaves 1.5 / 4.5).
constexpr int kVariants = 11;
constexpr int kVarW4[kVariants] = {1, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0};
constexpr int kVarCfg[kVariants] = {1, 1, 1, 2, 3, 4, 5, 6, 0, 7, 8};

// The kernel a (w4, cfg) pair launches for a shape on a device with `cus` compute units (MMR_GEMM_ROUTE_* of
// mmr.h): the one definition of the guards; launch() switches over it and mmr_linear_bf16_route reports it.
int route(int64_t m, int n, int k, bool hr, int w4, int cfg, int cus) {
  // big tiles when the grid still fills >= ~2 rounds of 256 CUs and K is deep enough
  const int64_t t256 = mmr::ceil_div(m, 256);
  // the persistent 4-wave kernel for epilogues without a residual (its 1-wave-per-SIMD epilogue
  // cannot hide a residual tile's fetch; 128x128 wave tiles: no registers left for a residual tile);
  // residual GEMMs keep the 8-wave kernels
  if (w4 && !hr && k >= 256 && k % 64 == 0 && m >= 4096) {
    // persistent grid: a multiple of 8 workgroups (one per CU), tiles split evenly per XCD
    const int grid = std::max(8, cus / 8 * 8);
    if (w4 == 1 && n % 256 == 0 && (t256 * (n / 256)) % grid == 0) return MMR_GEMM_ROUTE_W4_256X256;
    if (n % 192 == 0) return MMR_GEMM_ROUTE_W4_256X192;
  }
  if (cfg >= 7 && k % 128 == 0 && m % 256 == 0) {  // persistent 8-phase: 7 -> 256x256, 8 -> 256x192
    if (cfg == 7 && n % 256 == 0) return MMR_GEMM_ROUTE_P8_256X256;
    if (cfg == 8 && n % 192 == 0) return MMR_GEMM_ROUTE_P8_256X192;
  }
  if (cfg != 0 && k >= 256 && m >= 4096) {
    if (cfg <= 2 && n % 256 == 0 && t256 * (n / 256) >= 512)
      return cfg == 1 ? MMR_GEMM_ROUTE_BIG_256X256_KB64X2 : MMR_GEMM_ROUTE_BIG_256X256_KB32X4;
    if (cfg == 6 && n % 192 == 0 && t256 * (n / 192) >= 256) return MMR_GEMM_ROUTE_BIG_256X192_KB64X2;
    // 256x128, KB=32: 2 workgroups per CU (epilogue overlap)
    if (cfg >= 4 && cfg <= 5 && n % 128 == 0)
      return cfg == 4 ? MMR_GEMM_ROUTE_BIG_256X128_KB32X2 : MMR_GEMM_ROUTE_BIG_256X128_KB32X3;
    if (n % 128 == 0 && t256 * (n / 128) >= 512) return MMR_GEMM_ROUTE_BIG_256X128_KB64X3;
  }
  return MMR_GEMM_ROUTE_BASE_128X128;
}

// The one launch of gemm_bf16_tn_big: one workgroup per (WM MT 16) x (WN NT 16) tile, KB-deep slices through a
// STAGES-deep LDS ring (or the epilogue staging, whichever is larger); OCC = 2: two workgroups per CU
struct BigArgs {
  const uint16_t* x;
  const uint16_t* w;
  const float* b;
  const uint16_t* r;
  uint16_t* y;
  int64_t m;
  int n, k;
};
template <int WM, int WN, int MT, int NT, int KB, int STAGES, int OCC, int ACT, bool HB, bool HR>
void launch_big(const BigArgs& a, hipStream_t st) {
  constexpr int TBM = WM * MT * 16, TBN = WN * NT * 16;
  const int tm = (int)mmr::ceil_div(a.m, TBM), tn = a.n / TBN;
  const size_t lds = std::max<size_t>(STAGES * (TBM + TBN) * KB * 2, EPI_BIG_B);
  gemm_bf16_tn_big<WM, WN, MT, NT, KB, STAGES, ACT, HB, HR, OCC>
      <<<dim3(tm * tn), dim3(512), lds, st>>>(a.x, a.w, a.b, a.r, a.y, a.m, a.n, a.k, tm, tn);
}

template <int ACT, bool HB, bool HR>
void launch(const uint16_t* x, const uint16_t* w, const float* b, const uint16_t* r, uint16_t* y,
            int64_t m, int n, int k, hipStream_t st, int w4, int cfg) {
  const int tm = (int)mmr::ceil_div(m, 256);  // row tiles of the persistent routes
  const BigArgs ba{x, w, b, r, y, m, n, k};
  switch (route(m, n, k, HR, w4, cfg, cu_count())) {
    case MMR_GEMM_ROUTE_W4_256X256:
      if constexpr (!HR) {  // (the route takes no residual)
        // persistent grid: a multiple of 8 workgroups (one per CU), tiles split evenly per XCD
        const int grid = std::max(8, cu_count() / 8 * 8), tn = n / 256;
        gemm_bf16_tn_w4<8, ACT, HB, HR><<<dim3(std::min<int64_t>(grid, (int64_t)tm * tn)), dim3(256), w4_lds_bytes<8>(), st>>>(x, w, b, r, y, m, n, k, tm, tn);
      }
      return;
    case MMR_GEMM_ROUTE_W4_256X192: {
      const int grid = std::max(8, cu_count() / 8 * 8), tn = n / 192;
      gemm_bf16_tn_w4<6, ACT, HB, HR><<<dim3(std::min<int64_t>(grid, (int64_t)tm * tn)), dim3(256), w4_lds_bytes<6>(), st>>>(x, w, b, r, y, m, n, k, tm, tn);
      return;
    }
    case MMR_GEMM_ROUTE_P8_256X256:
    case MMR_GEMM_ROUTE_P8_256X192: {
      P8Args a;
      a.x = x, a.w = w, a.bias = b, a.r = r, a.y = y, a.m = m, a.n = n, a.k = k;
      a.ntst = p8_nt(m, n, 2);
      if (cfg == 7) return launch_p8<4, ACT, HB, HR>(a, st);
      return launch_p8<3, ACT, HB, HR>(a, st);
    }
    case MMR_GEMM_ROUTE_BIG_256X256_KB64X2: return launch_big<2, 4, 8, 4, 64, 2, 1, ACT, HB, HR>(ba, st);
    case MMR_GEMM_ROUTE_BIG_256X256_KB32X4: return launch_big<2, 4, 8, 4, 32, 4, 1, ACT, HB, HR>(ba, st);
    case MMR_GEMM_ROUTE_BIG_256X192_KB64X2: return launch_big<2, 4, 8, 3, 64, 2, 1, ACT, HB, HR>(ba, st);
    case MMR_GEMM_ROUTE_BIG_256X128_KB32X2: return launch_big<4, 2, 4, 4, 32, 2, 2, ACT, HB, HR>(ba, st);
    case MMR_GEMM_ROUTE_BIG_256X128_KB32X3: return launch_big<4, 2, 4, 4, 32, 3, 2, ACT, HB, HR>(ba, st);
    case MMR_GEMM_ROUTE_BIG_256X128_KB64X3: return launch_big<4, 2, 4, 4, 64, 3, 1, ACT, HB, HR>(ba, st);
    default: {
      const int bm = (int)mmr::ceil_div(m, BM), bn = (int)mmr::ceil_div(n, BN);
      gemm_bf16_tn<ACT, HB, HR><<<dim3(bm * bn), dim3(256), 0, st>>>(x, w, b, r, y, m, n, k, bm, bn);
    }
  }
}

// Per-shape variant choice: the first call with a (M, N, K, epilogue) key times every variant on
// the caller's stream (HIP events, 3 launches each after one warm-up) and keeps the fastest for
// the rest of the process — tile shape / persistence / pipeline depth trade off differently per
// shape (K = 96 ... 3072, N = 96 ... 3072).  Skipped (default variant) while the stream is being
// captured or when the output aliases an input.  mmr_pin_variant(MMR_PIN_GEMM_BF16, v) pins one
// variant for the process (tests / A/B tools).
struct TuneKey {
  int64_t m;
  int n, k, act, hb, hr;
  bool operator<(const TuneKey& o) const {
    if (m != o.m) return m < o.m;
    if (n != o.n) return n < o.n;
    if (k != o.k) return k < o.k;
    if (act != o.act) return act < o.act;
    if (hb != o.hb) return hb < o.hb;
    return hr < o.hr;
  }
};
std::mutex g_tune_mu;
std::map<std::pair<int, TuneKey>, int> g_tuned;  // (device, key) -> variant

template <class Run>
int tuned_variant(int64_t m, int n, int k, int act, bool hb, bool hr, const void* x, const void* r, const void* y,
                  hipStream_t st, Run&& run) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  const auto key = std::make_pair(dev, TuneKey{m, n, k, act, (int)hb, (int)hr});
  {
    std::lock_guard<std::mutex> lk(g_tune_mu);
    auto it = g_tuned.find(key);
    if (it != g_tuned.end()) return it->second;
  }
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return 0;
  if (y == x || y == r) return 0;
  hipEvent_t e0, e1;
  if (hipEventCreate(&e0) != hipSuccess) return 0;
  if (hipEventCreate(&e1) != hipSuccess) {
    (void)hipEventDestroy(e0);
    return 0;
  }
  // two interleaved passes, the faster of each variant's two timings: one 3-launch timing picked a
  // 13 % slower variant for the BERT QKV shape on some runs (clock / cache state of the moment)
  float vbest[kVariants];
  for (int v = 0; v < kVariants; ++v) vbest[v] = 1e30f;
  for (int pass = 0; pass < 2; ++pass)
    for (int v = 0; v < kVariants; ++v) {
      run(kVarW4[v], kVarCfg[v]);
      (void)hipEventRecord(e0, st);
      for (int rep = 0; rep < 3; ++rep) run(kVarW4[v], kVarCfg[v]);
      (void)hipEventRecord(e1, st);
      float ms = 1e30f;
      if (hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess)
        vbest[v] = std::min(vbest[v], ms);
    }
  float best = 1e30f;
  int bv = 0;
  for (int v = 0; v < kVariants; ++v)
    if (vbest[v] < best) {
      best = vbest[v];
      bv = v;
    }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  std::lock_guard<std::mutex> lk(g_tune_mu);
  g_tuned[key] = bv;
  return bv;
}

}  // namespace

#ifdef MMR_P8_STAMPS
extern "C" int mmr_diag_p8_stamps(unsigned long long* out, int64_t n) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(p8_stamps), (size_t)std::min<int64_t>(n, 1024 * 256) * 8) == hipSuccess ? 0 : 1;
}
#endif

extern "C" int32_t mmr_linear_bf16_n_variants(void) { return kVariants; }

extern "C" int32_t mmr_linear_bf16_variant(int64_t m, int32_t n, int32_t k, int32_t act, int32_t has_bias,
                                           int32_t has_residual) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return -1;
  std::lock_guard<std::mutex> lk(g_tune_mu);
  auto it = g_tuned.find(std::make_pair(dev, TuneKey{m, n, k, act, has_bias ? 1 : 0, has_residual ? 1 : 0}));
  return it == g_tuned.end() ? -1 : it->second;
}

extern "C" int32_t mmr_linear_bf16_route(int64_t m, int32_t n, int32_t k, int32_t has_residual, int32_t variant,
                                         int32_t cus) {
  if (m <= 0 || n <= 0 || k <= 0 || k % 8 != 0 || n % 8 != 0 || variant < 0 || variant >= kVariants) return -1;
  return route(m, n, k, has_residual != 0, kVarW4[variant], kVarCfg[variant], cus > 0 ? cus : cu_count());
}

extern "C" mmr_status mmr_linear_bf16(const uint16_t* x, const uint16_t* w, const float* bias,
                                      const uint16_t* residual, uint16_t* y, int64_t m, int32_t n,
                                      int32_t k, int32_t act, void* stream) {
  mmr::clear_error();
  MMR_REQUIRE(x && w && y, "mmr_linear_bf16: NULL pointer");
  MMR_REQUIRE(m >= 0 && n > 0 && k > 0, "mmr_linear_bf16: bad shape");
  MMR_REQUIRE(k % 8 == 0 && n % 8 == 0, "mmr_linear_bf16: K=%d and N=%d must be multiples of 8", k, n);
  MMR_REQUIRE(act == 0 || act == 1, "mmr_linear_bf16: act=%d", act);
  MMR_REQUIRE(mmr::ceil_div(m, BM) * mmr::ceil_div(n, BN) < (int64_t(1) << 31), "mmr_linear_bf16: grid too large");
  if (m == 0) return MMR_OK;
  hipStream_t st = mmr::as_stream(stream);
  const bool hb = bias != nullptr, hr = residual != nullptr;
  auto run = [&](int w4, int cfg) {
    mmr::pick_flags([&](auto a, auto b, auto r) { launch<a(), b(), r()>(x, w, bias, residual, y, m, n, k, st, w4, cfg); },
                    act != 0, hb, hr);
  };
  // the pinned variant (mmr_pin_variant), else the shape's tuned variant (tuned once per process on
  // the first call with that shape)
  const int pin = mmr::pin_gemm_bf16.load(std::memory_order_relaxed);
  const int v = (pin >= 0 && pin < kVariants) ? pin : tuned_variant(m, n, k, act, hb, hr, x, residual, y, st, run);
  run(kVarW4[v], kVarCfg[v]);
  MMR_LAUNCH_CHECK();
  return MMR_OK;
}

namespace {
// the tile width of the LayerNorm-fused GEMMs: 256 x 192 or 256 x 256, whichever fills whole rounds of
// the CUs (N = 768: 192 -> 512 tiles at M = 32768; 2304: 192; 3072: 256), ties to 256
int ln_nt(int64_t m, int n) {
  const bool ok3 = n % 192 == 0, ok4 = n % 256 == 0;
  if (!ok3 || !ok4) return ok4 ? 4 : (ok3 ? 3 : 0);
  const int64_t cus = std::max(8, cu_count() / 8 * 8), tm = m / 256;
  auto eff = [&](int nt) {
    const int64_t tiles = tm * (n / (64 * nt));
    return (double)tiles / (double)(mmr::ceil_div(tiles, cus) * cus);
  };
  return eff(3) > eff(4) + 1e-9 ? 3 : 4;
}

template <int NT, int ACT, bool HR, int LNM, bool STO>
void launch_ln(const uint16_t* x, const uint16_t* w, const float* b, const uint16_t* r, uint16_t* y, int64_t m,
               int n, int k, const float* lc, const float* v1, const float* v2, float* sp, hipStream_t st) {
  P8Args a;
  a.x = x, a.w = w, a.bias = b, a.r = r, a.y = y, a.m = m, a.n = n, a.k = k;
  a.ntst = p8_nt(m, n, 2);
  a.lc = lc, a.v1 = v1, a.v2 = v2, a.sp = sp;
  launch_p8<NT, ACT, true, HR, false, false, 0, LNM, STO>(a, st);
}

// ---- fp32-faithful (x3) linears on the 8-phase GEMM: Y = X W^T + b with f32 accumulation over the split
// operands X = [x_hi | x_lo] and W = [w_hi | w_lo] (bf16 rows, each segment kp = K padded to 128 with
// zeros): x_hi.w_hi + x_hi.w_lo + x_lo.w_hi, the three-term split of csrc/x3.hip, as ONE 8-phase GEMM
// whose K-tiles hold 32 k of both segments and whose MFMA segments issue the three products (X3P).
// x3_split_rows writes X (4 bytes per element of x).
template <bool VEC>
__global__ __launch_bounds__(256) void x3_split_rows(const float* __restrict__ x, int64_t ldx, int64_t m, int k, int kp,
                                                     uint16_t* __restrict__ xs) {
  const int g8 = kp / 8;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= m * g8) return;
  const int64_t row = t / g8;
  const int c0 = (int)(t % g8) * 8;
  const float* xr = x + row * ldx;
  float v[8];
  if (VEC && c0 + 8 <= k) {
    const float4 a = *(const float4*)(xr + c0), b = *(const float4*)(xr + c0 + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = c0 + e < k ? xr[c0 + e] : 0.f;
  }
  uint32_t hi[4], lo[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    hi[e] = mmr::pack2bf(v[2 * e], v[2 * e + 1]);
    lo[e] = mmr::pack2bf(v[2 * e] - __uint_as_float(hi[e] << 16), v[2 * e + 1] - __uint_as_float(hi[e] & 0xFFFF0000u));
  }
  uint16_t* o = xs + row * 2 * kp + c0;
  *(uint4*)o = make_uint4(hi[0], hi[1], hi[2], hi[3]);
  *(uint4*)(o + kp) = make_uint4(lo[0], lo[1], lo[2], lo[3]);
}

template <int NT, int ACT, bool HB, bool HR, bool OSPL = false>
void launch_x3p8(const uint16_t* xs, const uint16_t* w2, const float* b, const float* r, void* y, int64_t m, int npad,
                 int n, int kp, hipStream_t st) {
  P8Args a;
  a.x = xs, a.w = w2, a.bias = b, a.r = (const uint16_t*)r, a.y = (uint16_t*)y, a.m = m, a.n = npad, a.k = 2 * kp;
  a.ldn = n;
  launch_p8<NT, ACT, HB, HR, false, false, 0, 0, false, true, OSPL, true>(a, st);
}
}  // namespace

namespace {
// row statistics -> LayerNorm coefficients (rstd, -mean rstd).  part[row][np] = (sum, M2) of np equal
// parts of n / np columns each; merged with Chan's parallel formula: mean = sum / n, M2 = sum_p M2_p +
// (n / np) sum_p (mean_p - mean)^2 — no E[y^2] - mean^2 cancellation.  8 lanes per row, 2 parts each
// per step (np % 2 == 0), two passes over the (L2-resident) parts, reduced by xor swaps.
__global__ __launch_bounds__(256) void ln_row_coef(const float* __restrict__ part, int64_t m, int np, float inv_n,
                                                   float eps, float* __restrict__ coef) {
  const int64_t row = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 3;
  const int sub = threadIdx.x & 7;
  const float* p = part + (row < m ? row : 0) * np * 2;
  const float cnt = 1.0f / (inv_n * np), inv_cnt = inv_n * np;  // columns per part
  float s1 = 0.f;
  for (int q = 2 * sub; q < np; q += 16) {
    const float4 v = *(const float4*)(p + 2 * q);
    s1 += v.x + v.z;
  }
#pragma unroll
  for (int o = 1; o < 8; o <<= 1) s1 += __shfl_xor(s1, o, 64);
  const float mean = s1 * inv_n;
  float m2 = 0.f, dm = 0.f;
  for (int q = 2 * sub; q < np; q += 16) {
    const float4 v = *(const float4*)(p + 2 * q);
    const float d0 = v.x * inv_cnt - mean, d1 = v.z * inv_cnt - mean;
    m2 += v.y + v.w;
    dm = fmaf(d0, d0, fmaf(d1, d1, dm));
  }
#pragma unroll
  for (int o = 1; o < 8; o <<= 1) {
    m2 += __shfl_xor(m2, o, 64);
    dm += __shfl_xor(dm, o, 64);
  }
  if (row < m && sub == 0) {
    const float rstd = rsqrtf(fmaf(cnt, dm, m2) * inv_n + eps);
    *(float2*)(coef + 2 * row) = make_float2(rstd, -mean * rstd);
  }
}
}  // namespace

extern "C" mmr_status mmr_ln_row_coef(const float* stats, int64_t m, int32_t nparts, int32_t n, float eps, float* coef,
                                      void* stream) {
  mmr::clear_error();
  MMR_REQUIRE(stats && coef, "mmr_ln_row_coef: NULL pointer");
  MMR_REQUIRE(m >= 0 && nparts > 0 && nparts % 2 == 0 && n > 0 && n % nparts == 0,
              "mmr_ln_row_coef: m=%lld nparts=%d n=%d (nparts even, equal parts of n / nparts columns)", (long long)m,
              nparts, n);
  MMR_REQUIRE(aligned16(stats) && ((uintptr_t)coef & 7u) == 0, "mmr_ln_row_coef: alignment");
  if (m == 0) return MMR_OK;
  ln_row_coef<<<dim3((unsigned)mmr::ceil_div(m * 8, 256)), dim3(256), 0, mmr::as_stream(stream)>>>(stats, m, nparts,
                                                                                              1.0f / (float)n, eps, coef);
  MMR_LAUNCH_CHECK();
  return MMR_OK;
}

extern "C" int32_t mmr_linear_bf16_ln_parts(int64_t m, int32_t n, int32_t ln_mode) {
  const int nt = ln_mode == 2 ? (n % 192 == 0 ? 3 : 0) : ln_nt(m, n);
  return nt ? 4 * (n / (64 * nt)) : 0;
}

extern "C" int32_t mmr_x3_p8_kpad(int32_t k) { return k > 0 && k <= 4096 ? (k + 127) / 128 * 128 : 0; }

extern "C" int32_t mmr_x3_p8_npad(int32_t n) {
  if (n <= 0 || n > 16384 || n % 4) return 0;
  return n % 192 == 0 || n % 256 == 0 ? n : (n + 191) / 192 * 192;
}

extern "C" mmr_status mmr_x3_split_rows(const float* x, int64_t ldx, int64_t m, int32_t k, uint16_t* xs, void* stream) {
  mmr::clear_error();
  MMR_REQUIRE(x && xs, "mmr_x3_split_rows: NULL pointer");
  const int kp = mmr_x3_p8_kpad(k);
  MMR_REQUIRE(kp > 0 && m >= 0 && ldx >= k, "mmr_x3_split_rows: m=%lld k=%d ldx=%lld", (long long)m, k, (long long)ldx);
  if (m == 0) return MMR_OK;
  const int64_t n8 = m * (kp / 8);
  const dim3 grid((unsigned)mmr::ceil_div(n8, 256));
  hipStream_t st = mmr::as_stream(stream);
  if (aligned16(x) && ldx % 4 == 0 && k % 8 == 0)
    x3_split_rows<true><<<grid, 256, 0, st>>>(x, ldx, m, k, kp, xs);
  else
    x3_split_rows<false><<<grid, 256, 0, st>>>(x, ldx, m, k, kp, xs);
  MMR_LAUNCH_CHECK();
  return MMR_OK;
}

extern "C" mmr_status mmr_x3_linear_p8(const uint16_t* xs, const uint16_t* w2, const float* bias, const float* residual,
                                       void* y, int64_t m, int32_t n, int32_t k, int32_t act, int32_t out_hilo,
                                       void* stream) {
  mmr::clear_error();
  MMR_REQUIRE(xs && w2 && y, "mmr_x3_linear_p8: NULL pointer");
  const int kp = mmr_x3_p8_kpad(k);
  MMR_REQUIRE(kp > 0 && m > 0 && m % 256 == 0, "mmr_x3_linear_p8: m=%lld (multiple of 256), k=%d", (long long)m, k);
  const int npad = mmr_x3_p8_npad(n);
  MMR_REQUIRE(npad > 0, "mmr_x3_linear_p8: n=%d (multiple of 4, <= 16384)", n);
  MMR_REQUIRE(act == 0 || act == 1, "mmr_x3_linear_p8: act=%d", act);
  MMR_REQUIRE(!out_hilo || (n % 384 == 0 && residual == nullptr),
              "mmr_x3_linear_p8: split output needs n %% 384 == 0 and no residual (n=%d)", n);
  // (residual == y is fine: every output element is read, then written, by the one lane that owns it)
  hipStream_t st = mmr::as_stream(stream);
  const int nt = out_hilo ? 3 : (npad % 192 == 0 && npad % 256 == 0 ? ln_nt(m, npad) : (npad % 256 == 0 ? 4 : 3));
  const bool hb = bias != nullptr, hr = residual != nullptr;
  if (out_hilo)  // split output: 256 x 192 tiles, no residual
    mmr::pick_flags([&](auto a, auto b) { launch_x3p8<3, a(), b(), false, true>(xs, w2, bias, nullptr, y, m, npad, n, kp, st); },
                    act != 0, hb);
  else
    mmr::pick<3, 4>(nt, [&](auto t) {
      mmr::pick_flags(
          [&](auto a, auto b, auto r) {
            launch_x3p8<decltype(t)::value, a(), b(), r()>(xs, w2, bias, residual, y, m, npad, n, kp, st);
          },
          act != 0, hb, hr);
    });
  MMR_LAUNCH_CHECK();
  return MMR_OK;
}

extern "C" mmr_status mmr_linear_bf16_ln(const uint16_t* x, const uint16_t* w, const float* bias,
                                         const uint16_t* residual, uint16_t* y, int64_t m, int32_t n, int32_t k,
                                         int32_t act, int32_t ln_mode, const float* ln_coef, const float* ln_v1,
                                         const float* ln_v2, float* stats_out, void* stream) {
  mmr::clear_error();
  MMR_REQUIRE(x && w && bias && y, "mmr_linear_bf16_ln: NULL pointer");
  MMR_REQUIRE(m > 0 && m % 256 == 0 && k > 0 && k % 128 == 0,
              "mmr_linear_bf16_ln: m=%lld (multiple of 256), k=%d (multiple of 128)", (long long)m, k);
  const int nt = ln_nt(m, n);
  MMR_REQUIRE(n > 0 && nt != 0, "mmr_linear_bf16_ln: n=%d (multiple of 192 or 256)", n);
  MMR_REQUIRE(act == 0 || act == 1, "mmr_linear_bf16_ln: act=%d", act);
  MMR_REQUIRE(ln_mode >= 0 && ln_mode <= 2, "mmr_linear_bf16_ln: ln_mode=%d", ln_mode);
  MMR_REQUIRE(ln_mode == 0 || (ln_coef && ln_v1 && (ln_mode == 1 || ln_v2)),
              "mmr_linear_bf16_ln: ln_mode=%d needs the row coefficients and its column vectors", ln_mode);
  MMR_REQUIRE(ln_mode != 2 || residual, "mmr_linear_bf16_ln: ln_mode 2 normalises the residual");
  MMR_REQUIRE(!stats_out || act == 0, "mmr_linear_bf16_ln: row statistics only without GELU");
  hipStream_t st = mmr::as_stream(stream);
  const bool hr = residual != nullptr, so = stats_out != nullptr;
  // the combinations the BERT layer uses (towers.py): QKV / FFN1 (fold, + GELU for FFN1), O-proj /
  // FFN2 (normalised or plain residual, row statistics out)
  auto ln = [&](auto t, auto a, auto r, auto lm, auto s) {  // (NT, ACT, HR, LNM, STO)
    launch_ln<decltype(t)::value, decltype(a)::value, decltype(r)::value, decltype(lm)::value, decltype(s)::value>(
        x, w, bias, residual, y, m, n, k, ln_coef, ln_v1, ln_v2, stats_out, st);
  };
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  using I2 = std::integral_constant<int, 2>;
  using I3 = std::integral_constant<int, 3>;
  if (ln_mode == 1 && !hr && !so) {
    mmr::pick<3, 4>(nt, [&](auto t) {
      mmr::pick<0, 1>(act, [&](auto a) { ln(t, a, std::false_type{}, I1{}, std::false_type{}); });
    });
  } else if (ln_mode == 2 && act == 0) {
    // 256 x 192 tiles only: the 256 x 256 form of the normalised residual exceeds 256 VGPRs (a spill
    // in this kernel would also skew the K loop's counted vmcnt waits)
    MMR_REQUIRE(n % 192 == 0, "mmr_linear_bf16_ln: ln_mode 2 needs n %% 192 == 0 (n=%d)", n);
    mmr::pick_flags([&](auto s) { ln(I3{}, I0{}, std::true_type{}, I2{}, s); }, so);
  } else if (ln_mode == 0 && act == 0 && so) {
    mmr::pick<3, 4>(nt, [&](auto t) { mmr::pick_flags([&](auto r) { ln(t, I0{}, r, I0{}, std::true_type{}); }, hr); });
  } else {
    mmr::set_error("mmr_linear_bf16_ln: ln_mode=%d act=%d residual=%d stats_out=%d not built", ln_mode, act, (int)hr,
                   (int)so);
    return MMR_ERR_UNSUPPORTED;
  }
  MMR_LAUNCH_CHECK();
  return MMR_OK;
}

extern "C" mmr_status mmr_quantize_mxfp8(const uint16_t* x, int64_t rows, int32_t k, int32_t kp, int32_t layout,
                                         uint8_t* q, uint8_t* scales, void* stream) {
  mmr::clear_error();
  MMR_REQUIRE(x && q && scales, "mmr_quantize_mxfp8: NULL pointer");
  MMR_REQUIRE(layout >= 0 && layout <= 2, "mmr_quantize_mxfp8: layout=%d (0: X panels of 256 rows, 1 / 2: W panels of 192 / 256)", layout);
  const int pr = layout == 1 ? 192 : 256;
  MMR_REQUIRE(rows > 0 && rows % pr == 0, "mmr_quantize_mxfp8: rows=%lld must be a multiple of %d", (long long)rows, pr);
  MMR_REQUIRE(k > 0 && k % 8 == 0 && kp >= k && kp % 256 == 0, "mmr_quantize_mxfp8: k=%d kp=%d (k %% 8 == 0, kp >= k, kp %% 256 == 0)", k, kp);
  const int64_t threads = rows * (kp / 16);
  hipStream_t st = mmr::as_stream(stream);
  const dim3 grid((unsigned)mmr::ceil_div(threads, 256));
  if (layout == 0) quantize_mxfp8<0><<<grid, dim3(256), 0, st>>>(x, rows, k, kp, q, scales);
  else if (layout == 1) quantize_mxfp8<1><<<grid, dim3(256), 0, st>>>(x, rows, k, kp, q, scales);
  else quantize_mxfp8<2><<<grid, dim3(256), 0, st>>>(x, rows, k, kp, q, scales);
  MMR_LAUNCH_CHECK();
  return MMR_OK;
}

extern "C" mmr_status mmr_linear_mxfp8(const uint8_t* xq, const uint8_t* xs, const uint8_t* wq, const uint8_t* ws,
                                       int32_t w_layout, const float* bias, const uint16_t* residual, uint16_t* y,
                                       int64_t m, int32_t n, int32_t kp, int32_t act, void* stream) {
  mmr::clear_error();
  MMR_REQUIRE(xq && xs && wq && ws && y, "mmr_linear_mxfp8: NULL pointer");
  MMR_REQUIRE(w_layout == 1 || w_layout == 2, "mmr_linear_mxfp8: w_layout=%d (1: 192-row W panels, 2: 256-row)", w_layout);
  const int tbn = w_layout == 1 ? 192 : 256;
  MMR_REQUIRE(m > 0 && m % 256 == 0, "mmr_linear_mxfp8: m=%lld must be a positive multiple of 256", (long long)m);
  MMR_REQUIRE(n > 0 && n % tbn == 0, "mmr_linear_mxfp8: n=%d must be a positive multiple of %d", n, tbn);
  MMR_REQUIRE(kp > 0 && kp % 256 == 0, "mmr_linear_mxfp8: kp=%d must be a positive multiple of 256", kp);
  MMR_REQUIRE(act == 0 || act == 1, "mmr_linear_mxfp8: act=%d", act);
  hipStream_t st = mmr::as_stream(stream);
  P8Args a;
  a.x = (const uint16_t*)xq, a.w = (const uint16_t*)wq, a.bias = bias, a.r = residual, a.y = y, a.m = m, a.n = n, a.k = kp;
  a.xs = xs, a.ws = ws;
  a.ntst = p8_nt(m, n, 2);
  mmr::pick<3, 4>(tbn / 64, [&](auto t) {
    mmr::pick_flags([&](auto ac, auto hb, auto hr) { launch_p8<decltype(t)::value, ac(), hb(), hr(), true>(a, st); },
                    act != 0, bias != nullptr, residual != nullptr);
  });
  MMR_LAUNCH_CHECK();
  return MMR_OK;
}

extern "C" mmr_status mmr_linear_mxfp8_q8(const uint8_t* xq, const uint8_t* xs, const uint8_t* wq, const uint8_t* ws,
                                         const float* bias, uint8_t* yq, uint8_t* ys, int64_t m, int32_t n,
                                         int32_t kp, int32_t act, void* stream) {
  mmr::clear_error();
  MMR_REQUIRE(xq && xs && wq && ws && yq && ys, "mmr_linear_mxfp8_q8: NULL pointer");
  MMR_REQUIRE(m > 0 && m % 256 == 0, "mmr_linear_mxfp8_q8: m=%lld must be a positive multiple of 256", (long long)m);
  MMR_REQUIRE(n > 0 && n % 256 == 0, "mmr_linear_mxfp8_q8: n=%d must be a positive multiple of 256 (weights in layout 2)", n);
  MMR_REQUIRE(kp > 0 && kp % 256 == 0, "mmr_linear_mxfp8_q8: kp=%d must be a positive multiple of 256", kp);
  MMR_REQUIRE(act == 0 || act == 1, "mmr_linear_mxfp8_q8: act=%d", act);
  hipStream_t st = mmr::as_stream(stream);
  P8Args a;
  a.x = (const uint16_t*)xq, a.w = (const uint16_t*)wq, a.bias = bias, a.y = (uint16_t*)yq, a.m = m, a.n = n, a.k = kp;
  a.xs = xs, a.ws = ws, a.ys = ys;
  a.ntst = p8_nt(m, n, 1);
  mmr::pick_flags([&](auto ac, auto hb) { launch_p8<4, ac(), hb(), false, true, true>(a, st); }, act != 0, bias != nullptr);
  MMR_LAUNCH_CHECK();
  return MMR_OK;
}

namespace mmr {
// The fp16 kNN scan on the persistent 8-phase GEMM (gemm_bf16_tn_p8<KNN>): qh [256 tiles_m][K] fp16
// unit queries, row-major (zero rows past the pass; tiles_m 1-4), gh = the index's fp16 gallery in the
// tile32h layout, tiles_n * 256 rows (zero rows past nval); rs (optional) the per-row inverse norms of a
// raw-row gallery (NULL: unit rows); writes unit maxima of unit_rows (2 or 4) consecutive rows gm
// [256 tiles_m][ldG] (ldG >= tiles_n * 256 / unit_rows) and block maxima bm [256 tiles_m][ldB].
// K % 128 == 0 (the caller checks).
hipError_t knn_scan_p8(const uint16_t* qh, const uint16_t* gh, int K, int tiles_n, int64_t nval, float* gm,
                       int64_t ldG, float* bm, int64_t ldB, int unit_rows, hipStream_t st, int tiles_m,
                       const float* rs) {
  P8Args a;
  a.x = qh, a.w = gh, a.m = 256 * tiles_m, a.n = tiles_n * 256, a.k = K;
  a.gm = gm, a.bm = bm, a.ldg = ldG, a.ldb = ldB, a.nval = nval, a.rs = rs;
  if (unit_rows == 2) launch_p8<4, 0, false, false, false, false, 2>(a, st);
  else launch_p8<4, 0, false, false, false, false, 4>(a, st);
  return hipGetLastError();
}
}  // namespace mmr
