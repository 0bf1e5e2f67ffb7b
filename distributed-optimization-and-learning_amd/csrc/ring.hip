// ring.hip — the ring (circle-graph) mixes: one round, its fused DGD and EXTRA
// rounds, the two edge rows of a sharded ring, and eps rounds in one pass.
//
// Layout: agent k's parameter vector is row k of a row-major fp32 matrix
// with leading dimension ld (elements).  Columns are streamed 16 B per lane
// (f4) when every row base is 16-B aligned; otherwise, and for the
// P % 4 tail, the same kernels run on scalar columns.
//
// This file holds the default paths only.  Launch variants that were measured
// behind environment switches and dropped (8192 x 2^20 unless noted; all gave
// the default's bits unless noted; none was consistently faster; code last
// present at 1a824fc):
//   DOL_RING_DMA=0, DOL_RING_PF / _NT / _ROWS: the float4 ring mix staged in registers
//     (ring_mix_kernel<f4, ...>), 5.91 vs 6.17 TB/s for the LDS-DMA kernel; R = 64 tiles 5.1-5.4.
//   DOL_RING_NTI=0: the LDS-DMA ring mix without nontemporal interior-row loads,
//     11.15-11.16 vs 10.90-10.93 ms (profiles/r01d_ring_nti.txt).
//   DOL_RING_STREAM=1 as a process default, DOL_RING_STREAM_T / _PF / _NT / _LDS: ring_stream_kernel with 4 / 16
//     rows in flight, plain loads, other tile heights, an LDS occupancy cap (profiles/r03_eps_stream.txt; see
//     dol_mix_ring_steps_ex_f32 for the box A / C / E figures).  The kernel stays as variant 2.
//   DOL_RING_DMA_D=16: ring_stream_dma_kernel with a 16-row ring per wave, 12.53 vs 12.61 ms at 1024-row
//     tiles, 12.86 vs 12.81 at 8192 (profiles/r04c_eps_dma_sweep.jsonl).  DOL_RING_DMA_SYNC / _ORDER: variants 4 / 5.
//   DOL_RING_DMA_PROBE=1: that kernel as a copy (wrong results by design), as fast as the real one,
//     12.59 vs 12.61 ms: the pass is bound by its access pattern (same file).
// Switches that stay: DOL_DGD_EPI_NT (a runtime branch inside every DGD kernel, dol_launch.h) and
// dol_ring_steps_set_variant / variants 1-5 of dol_mix_ring_steps_ex_f32 (the product path's tuner picks).
#include <atomic>

#include "dol_launch.h"

namespace {
constexpr int kThreads = 256;            // 4 waves of 64
constexpr int kRingStepsVariants = 5;  // highest dol_mix_ring_steps_ex_f32 variant

// ----------------------------------------------------------------------------
// Ring mix, register-staged: one workgroup = one column tile (256 lanes x V)
// x rows_per_block consecutive agent rows.  The three-point stencil along the
// agent axis is carried in a register window; PF rows are loaded one iteration
// ahead.  Runs the scalar tail columns (V = float: P % 4, or unaligned rows)
// only; the float4 stream is ring_mix_dma_kernel's.
// Measured on MI355X (tools/membench*.hip, 8192 x 2^20): short-lived tiles win
// — 4 rows with all 6 loads issued up front (PF >= rows), plain loads and
// nontemporal stores reach 6.14 TB/s against a 6.26 TB/s flat-copy ceiling,
// while 64-row long-lived tiles stay near 5.1-5.4.  The halo rows (2 per
// tile) are re-read from L2: vertically adjacent tiles are n_col_tiles
// blocks apart (a multiple of 8 -> same XCD) and co-resident.
// ----------------------------------------------------------------------------
constexpr int kRingTailRows = 4;  // rows per block = rows loaded ahead

template <typename V, class Epi = NoEpi>
__global__ __launch_bounds__(kThreads) void ring_mix_kernel(
    const float* __restrict__ X, int64_t ldx, float* __restrict__ Y, int64_t ldy,
    int n_rows, int64_t c_off, int64_t ncols_v, int64_t n_col_tiles, int rows_per_block,
    const float* __restrict__ halo_prev, const float* __restrict__ halo_next,
    const float* __restrict__ wprev, const float* __restrict__ wnext, Epi epi) {
  // 32-bit block decomposition (grids are < 2^24 blocks); column tile fastest,
  // so co-resident workgroups share rows and the halo re-reads hit L2
  const uint32_t b = blockIdx.x;
  const uint32_t nct = static_cast<uint32_t>(n_col_tiles);
  const uint32_t ct = b % nct;
  const int rg = static_cast<int>(b / nct);
  const int64_t c = int64_t(ct) * kThreads + threadIdx.x;  // column in units of V
  if (c >= ncols_v) return;
  const int r0 = rg * rows_per_block;
  const int r1 = min(r0 + rows_per_block, n_rows);

  auto row = [&](int r) -> const V* {
    const float* base = (r < 0) ? halo_prev : (r >= n_rows ? halo_next : X + int64_t(r) * ldx);
    return reinterpret_cast<const V*>(base + c_off) + c;
  };

  constexpr int PF = kRingTailRows;
  V q[PF + 2];
  q[0] = *row(r0 - 1);
  q[1] = *row(r0);
#pragma unroll
  for (int k = 0; k < PF; ++k) q[2 + k] = *row(min(r0 + 1 + k, r1));

  for (int i = r0; i < r1; i += PF) {
    V nx[PF];
#pragma unroll
    for (int k = 0; k < PF; ++k) nx[k] = *row(min(i + PF + 1 + k, r1));
#pragma unroll
    for (int k = 0; k < PF; ++k) {
      const int r = i + k;
      if (r < r1) {
        V out = axpy0(wprev[r], q[k], wnext[r], q[k + 2]);
        const int64_t cf = c_off + c * Vec<V>::W;
        if constexpr (Epi::kCentre) out = epi.apply_centre(out, q[k + 1], epi.template load<V>(r, cf), r, cf);
        else out = epi.apply(out, epi.template load<V>(r, cf), r, cf);
        __builtin_nontemporal_store(out, reinterpret_cast<V*>(Y + int64_t(r) * ldy + c_off) + c);
      }
    }
    q[0] = q[PF];
    q[1] = q[PF + 1];
#pragma unroll
    for (int k = 0; k < PF; ++k) q[2 + k] = nx[k];
  }
}

// The two boundary rows of a sharded ring block in ONE launch (the multi-GPU
// round, dolhip.parallel.ShardedRing: the interior rows are mixed while the
// halo rows travel, then these two): blockIdx.y = 0 -> row 0 (previous row =
// halo_prev), 1 -> row n_rows - 1 (next row = halo_next); with n_rows == 1 only
// y = 0 runs and uses both halos.  Same arithmetic as ring_mix_kernel.
template <typename V, class Epi = NoEpi>
__global__ __launch_bounds__(kThreads) void ring_edges_kernel(
    const float* __restrict__ X, int64_t ldx, float* __restrict__ Y, int64_t ldy, int n_rows, int64_t c_off,
    int64_t ncols_v, const float* __restrict__ halo_prev, const float* __restrict__ halo_next,
    const float* __restrict__ wprev, const float* __restrict__ wnext, Epi epi) {
  const int64_t c = int64_t(blockIdx.x) * kThreads + threadIdx.x;
  if (c >= ncols_v) return;
  const int r = blockIdx.y == 0 ? 0 : n_rows - 1;
  const float* pv = r == 0 ? halo_prev : X + int64_t(r - 1) * ldx;
  const float* nx = r == n_rows - 1 ? halo_next : X + int64_t(r + 1) * ldx;
  const V a = reinterpret_cast<const V*>(pv + c_off)[c];
  const V b = reinterpret_cast<const V*>(nx + c_off)[c];
  V out = axpy0(wprev[r], a, wnext[r], b);
  const int64_t cf = c_off + c * Vec<V>::W;
  out = epi.apply(out, epi.template load<V>(r, cf), r, cf);
  reinterpret_cast<V*>(Y + int64_t(r) * ldy + c_off)[c] = out;
}

// LDS-DMA form of the ring mix (the default float4 path).  Each wave moves
// its 1 KiB quarter of the tile's R + 2 rows straight into LDS with
// global_load_lds_dwordx4 (default cache policy: the halo rows' second reads
// must hit L2), waits on its own vmcnt, reads its lanes back and stores with
// nontemporal stores.  No barrier: a wave only reads what it loaded.  On
// MI355X (tools/membench7/8.hip, same box): 6.17 TB/s vs 5.91 for the
// register-staged kernel, = the measured copy ceiling (6.16); nt loads on
// every row cost 17 % (they evict the halo rows from L2), but nt on the R - 2
// rows no other tile reads (NTI) gains 2.3 %: 10.90-10.93 vs 11.15-11.16 ms at
// 8192 x 2^20, three A/B pairs on one box (profiles/r01d_ring_nti.txt).  The
// same split in ring_steps_kernel gained nothing.

// COPY (roofline calibration only): the same loads, cache policies and stores,
// with the stencil replaced by the tile's own row (Y = X): the memory-system
// ceiling of exactly this kernel's access pattern.
// NTI is always true now; the parameter list stays <R, Epi, NTI, COPY> because
// bench.py reports the headline's kernel by that name
// (ring_mix_dma_kernel<4, NoEpi, true, false>).
template <int R, class Epi, bool NTI, bool COPY>
__global__ __launch_bounds__(kThreads) void ring_mix_dma_kernel(
    const float* __restrict__ X, int64_t ldx, float* __restrict__ Y, int64_t ldy, int n_rows,
    int64_t ncols_v, int64_t n_col_tiles, const float* __restrict__ halo_prev,
    const float* __restrict__ halo_next, const float* __restrict__ wprev, const float* __restrict__ wnext,
    Epi epi) {
  __shared__ __attribute__((aligned(16))) float lds[kThreads / 64][R + 2][256];
  const uint32_t b = blockIdx.x;
  const uint32_t nct = static_cast<uint32_t>(n_col_tiles);
  const uint32_t ct = b % nct;
  const int r0 = static_cast<int>(b / nct) * R;
  const int r1 = min(r0 + R, n_rows);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t c = int64_t(ct) * kThreads + threadIdx.x;  // f4 column
  if (c >= ncols_v) return;
  auto row = [&](int r) -> const float* {
    return (r < 0) ? halo_prev : (r >= n_rows ? halo_next : X + int64_t(r) * ldx);
  };
#pragma unroll
  for (int k = 0; k < R + 2; ++k) {
    const int r = min(r0 - 1 + k, r1);
    if (NTI && k >= 2 && k < R)  // rows no other tile reads: nontemporal
      __builtin_amdgcn_global_load_lds(DOL_GPTR(row(r) + 4 * c), DOL_LPTR(&lds[wave][k][0]), 16, 0, 2);
    else
      __builtin_amdgcn_global_load_lds(DOL_GPTR(row(r) + 4 * c), DOL_LPTR(&lds[wave][k][0]), 16, 0, 0);
  }
  decltype(epi.template load<f4>(0, 0)) es[R];  // epilogue operands ride with the DMA
#pragma unroll
  for (int k = 0; k < R; ++k) es[k] = epi.template load<f4>(min(r0 + k, r1 - 1), 4 * c);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  f4 v[R + 2];
#pragma unroll
  for (int k = 0; k < R + 2; ++k) v[k] = *reinterpret_cast<const f4*>(&lds[wave][k][lane * 4]);
#pragma unroll
  for (int k = 0; k < R; ++k) {
    const int r = r0 + k;
    if constexpr (Epi::kCentre) {  // the epilogue takes the row's own x from the tile
      if (r < r1)
        __builtin_nontemporal_store(epi.apply_centre(axpy0(wprev[r], v[k], wnext[r], v[k + 2]), v[k + 1], es[k], r, 4 * c),
                                    reinterpret_cast<f4*>(Y + int64_t(r) * ldy) + c);
    } else {
      if (r < r1)
        __builtin_nontemporal_store(COPY ? v[k + 1] : epi.apply(axpy0(wprev[r], v[k], wnext[r], v[k + 2]), es[k], r, 4 * c),
                                    reinterpret_cast<f4*>(Y + int64_t(r) * ldy) + c);
    }
  }
}

// ----------------------------------------------------------------------------
// Temporally blocked ring mix: STEPS synchronous rounds in one HBM pass
// (FedLCon's eps consensus steps, DIST/simulators.py:190-196).  A tile of R
// output rows loads R + 2*STEPS rows once and applies the 3-point stencil
// STEPS times in registers; level t is valid on [t, R + 2*STEPS - t).  Every
// intermediate uses the single-round formula (fl(fl(+0 + wp*a) + wn*b)), so the
// result is bit-identical to STEPS launches of ring_mix_kernel.  Wrap-around
// ring inside X (one shard).
// Tried (profiles/r02_ring_steps_eps_experiments.txt): intermediate levels as
// fma(wp, a, +0) + wn*b (three packed ops instead of four; exact up to -0 for
// +0 on the intermediate levels, the last level kept as axpy0 restores the bits)
// cut the pk ops per thread and tile 1,040 -> 824 but ran 12.63-12.74 vs
// 12.14-12.16 ms at eps = 5, three A/B pairs on one box: the pass is not
// VALU-issue bound.
// ----------------------------------------------------------------------------
template <int STEPS, int R, typename V = f4>
__global__ __launch_bounds__(kThreads) void ring_steps_kernel(
    const float* __restrict__ X, int64_t ldx, float* __restrict__ Y, int64_t ldy, int n_rows,
    int64_t ncols_v, uint32_t n_col_tiles, const float* __restrict__ wprev,
    const float* __restrict__ wnext, uint32_t n_row_tiles) {
  constexpr int L = R + 2 * STEPS;
  // XCD-aware order: the dispatcher deals blocks round-robin over the 8 XCDs,
  // so XCD x = b % 8 takes column tiles x, x + 8, ... and walks each one's row
  // tiles in order — a tile's 2*STEPS halo rows were just loaded by its
  // predecessor into the same L2.  (Column-tile-fastest order put vertical
  // neighbours a residency generation apart: 385 vs 431 rounds/s at eps = 5,
  // 8192 x 2^20.)
  const uint32_t b = blockIdx.x;
  const uint32_t x = b & 7u, l = b >> 3;
  const uint32_t ct = (l / n_row_tiles) * 8 + x;
  const int r0 = static_cast<int>(l % n_row_tiles) * R;
  if (ct >= n_col_tiles) return;
  const int64_t c = int64_t(ct) * kThreads + threadIdx.x;
  if (c >= ncols_v) return;
  auto wrap = [&](int r) { r %= n_rows; return r < 0 ? r + n_rows : r; };
  V v[L];
#pragma unroll
  for (int i = 0; i < L; ++i) v[i] = reinterpret_cast<const V*>(X + int64_t(wrap(r0 - STEPS + i)) * ldx)[c];
#pragma unroll
  for (int t = 1; t <= STEPS; ++t) {
    V prev_old = v[t - 1];
#pragma unroll
    for (int i = t; i < L - t; ++i) {
      const int g = wrap(r0 - STEPS + i);
      const V cur_old = v[i];
      v[i] = axpy0(wprev[g], prev_old, wnext[g], v[i + 1]);
      prev_old = cur_old;
    }
  }
#pragma unroll
  for (int i = 0; i < R; ++i) {
    const int r = r0 + i;
    if (r < n_rows) __builtin_nontemporal_store(v[STEPS + i], reinterpret_cast<V*>(Y + int64_t(r) * ldy) + c);
  }
}

// ----------------------------------------------------------------------------
// Streaming temporal blocking (r03): the same STEPS synchronous rounds and the
// same bits as ring_steps_kernel, with each thread walking ONE f4 column down
// a tile of T rows (+ STEPS halo rows on each side) instead of holding the
// whole tile in registers: when level-0 row i arrives, level t is produced at
// index i - t from level t-1's values at i - t + 1 (this step) and i - t - 1
// (two steps ago), so each level keeps its last two values (the step parity
// picks the register set: no copies) and the loads run PF rows ahead.  HBM
// sees one continuous read stream per column (halo re-reads 2 STEPS / T of
// the tile, from L2: vertically adjacent tiles run back to back on one XCD)
// instead of ring_steps_kernel's load-all / compute / store bursts with 2
// STEPS / R = 45 % halo at R = 22.  The stencil has no diagonal term (circle
// W: W_ii = 0), so only the two neighbours enter, as in axpy0.
// ----------------------------------------------------------------------------
template <int S, int PF, bool INTERIOR>
__device__ __forceinline__ void ring_stream_body(const f4* __restrict__ xc, int64_t ldv, float* __restrict__ Y,
                                                 int64_t ldy, int64_t c, int n_rows, int r0, int nT,
                                                 const float* __restrict__ wprev, const float* __restrict__ wnext) {
  const int nsteps = nT + 2 * S;
  auto wrap = [&](int g) {  // |g| within one ring length of [0, n_rows)
    if constexpr (!INTERIOR) g = g < 0 ? g + n_rows : (g >= n_rows ? g - n_rows : g);
    return g;
  };
  // the prefetch walks the input rows with a running pointer (one 64-bit add per
  // step, a wrap test on edge tiles); past the tile's last input row it stays on
  // that row (always valid, never used)
  int gl = wrap(r0 - S);
  const f4* lp = xc + int64_t(gl) * ldv;
  int left = nsteps;  // input rows not yet issued
  auto next = [&]() {
    const f4 v = __builtin_nontemporal_load(lp);
    if (--left > 0) {
      ++gl;
      lp += ldv;
      if constexpr (!INTERIOR) {
        if (gl == n_rows) {
          gl = 0;
          lp = xc;
        }
      }
    }
    return v;
  };
  f4 pf[PF];
#pragma unroll
  for (int u = 0; u < PF; ++u) pf[u] = next();
  f4 hA[S], hB[S];  // level t's value from two steps back, even / odd steps
#pragma unroll
  for (int t = 0; t < S; ++t) hA[t] = hB[t] = f4{0.f, 0.f, 0.f, 0.f};
  f4* yp = reinterpret_cast<f4*>(Y + int64_t(r0) * ldy) + c;  // the next output row
  const int64_t ldyv = ldy / 4;
  struct Wn { float v[PF + S]; };  // the weights of rows r0 - 2S + i0 .. (one scalar load per array and PF steps)
  for (int i0 = 0; i0 < nsteps; i0 += PF) {
    Wn wp, wn;
    if constexpr (INTERIOR) {
      wp = *reinterpret_cast<const Wn*>(wprev + (r0 - 2 * S + i0));
      wn = *reinterpret_cast<const Wn*>(wnext + (r0 - 2 * S + i0));
    } else {
#pragma unroll
      for (int j = 0; j < PF + S; ++j) {
        const int g = wrap(r0 - 2 * S + min(i0 + j, nsteps + S - 1));
        wp.v[j] = wprev[g];
        wn.v[j] = wnext[g];
      }
    }
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      const int i = i0 + u;
      f4 nv = pf[u];  // level 0 at index i
      pf[u] = next();
#pragma unroll
      for (int t = 1; t <= S; ++t) {
        f4& hv = (u & 1) ? hB[t - 1] : hA[t - 1];
        const f4 old = hv;  // level t-1 at index i - t - 1
        hv = nv;            // level t-1 at index i - t + 1, for two steps on
        // row of index i - t = r0 - 2S + i0 + (u + S - t)
        nv = axpy0(wp.v[u + S - t], old, wn.v[u + S - t], nv);
      }
      if (i >= 2 * S && i < nsteps) {  // level S at index i - S = row r0 + i - 2S
        __builtin_nontemporal_store(nv, yp);
        yp += ldyv;
      }
    }
  }
}

template <int S, int PF>
__global__ __launch_bounds__(kThreads) void ring_stream_kernel(
    const float* __restrict__ X, int64_t ldx, float* __restrict__ Y, int64_t ldy, int n_rows,
    int64_t ncols_v, uint32_t n_col_tiles, const float* __restrict__ wprev,
    const float* __restrict__ wnext, uint32_t n_row_tiles, int T) {
  static_assert(PF % 2 == 0, "the step parity selects the history registers");
  const uint32_t b = blockIdx.x;
  const uint32_t x = b & 7u, l = b >> 3;
  const uint32_t ct = (l / n_row_tiles) * 8 + x;
  const int r0 = static_cast<int>(l % n_row_tiles) * T;
  if (ct >= n_col_tiles) return;
  const int64_t c = int64_t(ct) * kThreads + threadIdx.x;
  if (c >= ncols_v) return;
  const int nT = min(T, n_rows - r0);
  const f4* xc = reinterpret_cast<const f4*>(X) + c;
  const int64_t ldv = ldx / 4;
  if (r0 - 2 * S >= 0 && r0 + nT + S + PF <= n_rows)  // every row and weight index in range
    ring_stream_body<S, PF, true>(xc, ldv, Y, ldy, c, n_rows, r0, nT, wprev, wnext);
  else
    ring_stream_body<S, PF, false>(xc, ldv, Y, ldy, c, n_rows, r0, nT, wprev, wnext);
}

// ----------------------------------------------------------------------------
// The streaming pass on the headline's load path (r04): the level arithmetic
// of ring_stream_body (same bits), with the input rows arriving by LDS-DMA
// (global_load_lds_dwordx4) into a per-wave ring of D 1-KiB rows instead of
// VGPRs.  Each wave streams its own 1 KiB column strip down the tile and reads
// back only what it loaded (no barrier; the covering vmcnt orders the wave's
// own reads), so D - 1 rows per wave stay in flight with no VGPR held for
// them.  Every step issues exactly one DMA and one store (buffer stores: the
// 2S prologue steps and the tail store out of range, dropped but counted;
// past the last input row the DMA re-reads that row into a consumed slot), so
// one wait, vmcnt(2D - 2), always retires exactly the row about to be read:
// after L(i) come D - 1 loads and D - 1 stores (the prologue pairs each of its
// D - 1 loads with a dropped store to keep that count from the first step).
// Halo rows (the first and last 2S of a tile) load with the default policy,
// so the neighbouring tile on the same XCD finds them in L2; the rest are
// nontemporal, as in ring_mix_dma_kernel.
// ----------------------------------------------------------------------------
template <int N>
__device__ __forceinline__ void vm_wait() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

template <int S, int D, int PF, bool INTERIOR, bool SYNC = false>
__device__ __forceinline__ void ring_stream_dma_body(const float* __restrict__ X, int64_t ldx, float* __restrict__ Y,
                                                     int64_t ldy, int64_t c, int n_rows, int r0, int nT,
                                                     const float* __restrict__ wprev,
                                                     const float* __restrict__ wnext, float* ring, bool live) {
  static_assert(D == PF || D == 2 * PF, "ring slots are compile-time within a chunk");
  static_assert(2 * D - 2 <= 63, "vmcnt is 6 bits");
  const int nsteps = nT + 2 * S;
  const int ntot = (nsteps + PF - 1) / PF * PF;  // steps run, the tail past nsteps included
  const int lane = threadIdx.x & 63;
  auto wrap = [&](int g) {
    if constexpr (!INTERIOR) g = g < 0 ? g + n_rows : (g >= n_rows ? g - n_rows : g);
    return g;
  };
  int gl = wrap(r0 - S);
  const float* xc = X + 4 * c;
  const float* lp = xc + int64_t(gl) * ldx;
  int issued = 0;
  auto issue = [&](int j) {  // input index j into slot j % D (j >= nsteps: the last row again)
    float* dst = ring + (j & (D - 1)) * 256;
    if (j < 2 * S || j >= nsteps - 2 * S)  // halo rows: default policy (re-read from L2 by the next tile)
      __builtin_amdgcn_global_load_lds(DOL_GPTR(lp), DOL_LPTR(dst), 16, 0, 0);
    else
      __builtin_amdgcn_global_load_lds(DOL_GPTR(lp), DOL_LPTR(dst), 16, 0, 2);
    if (++issued < nsteps) {
      ++gl;
      lp += ldx;
      if constexpr (!INTERIOR) {
        if (gl == n_rows) {
          gl = 0;
          lp = xc;
        }
      }
    }
  };
  const uint32_t voff = static_cast<uint32_t>(c) * 16u;
  auto store = [&](int i, f4 v) {  // output of step i: row r0 + i - 2S when 2S <= i < nsteps, else dropped
    const bool ok = live && i >= 2 * S && i < nsteps;
    const uint32_t oob = kOOB + (uint32_t(i + D) << 4);  // distinct dropped addresses: no two dummy stores merge
    const int r = ok ? r0 + i - 2 * S : r0;
    const rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(Y + int64_t(r) * ldy, 0, static_cast<int>(ldy * 4), 0x00020000);
    // nontemporal (2) and volatile (bit 31): the dropped stores must all be
    // issued -- the vmcnt accounting counts them -- and identical prologue
    // stores would otherwise be merged by dead-store elimination
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4, v), rs, ok ? voff : oob, 0, int(0x80000002u));
  };
#pragma unroll
  for (int j = 0; j < D - 1; ++j) {
    issue(j);
    store(j - D, f4{0.f, 0.f, 0.f, 0.f});
  }
  f4 hA[S], hB[S];
#pragma unroll
  for (int t = 0; t < S; ++t) hA[t] = hB[t] = f4{0.f, 0.f, 0.f, 0.f};
  struct Wn { float v[PF + S]; };
  for (int i0 = 0; i0 < ntot; i0 += PF) {
    // SYNC: the block's four waves meet once per chunk, so the four 1-KiB pieces
    // of each row are requested together (raw s_barrier: no vmcnt drain)
    if constexpr (SYNC) __builtin_amdgcn_s_barrier();
    Wn wp, wn;
    if constexpr (INTERIOR) {
      wp = *reinterpret_cast<const Wn*>(wprev + (r0 - 2 * S + i0));
      wn = *reinterpret_cast<const Wn*>(wnext + (r0 - 2 * S + i0));
    } else {
#pragma unroll
      for (int j = 0; j < PF + S; ++j) {
        const int g = wrap(r0 - 2 * S + min(i0 + j, nsteps + S - 1));
        wp.v[j] = wprev[g];
        wn.v[j] = wnext[g];
      }
    }
    const float* slot0 = ring + (D == PF ? 0 : (i0 & (D - 1))) * 256 + lane * 4;
#pragma unroll
    for (int u = 0; u < PF; ++u) {
      const int i = i0 + u;
      // keep the DMA below the previous step's read and store: the slot it
      // overwrites was read by that step (WAR), and the store order is counted
      asm volatile("" ::: "memory");
      issue(i + D - 1);
      vm_wait<2 * D - 2>();  // L(i) has landed
      f4 nv = *reinterpret_cast<const f4*>(slot0 + u * 256);  // level 0 at index i
#pragma unroll
      for (int t = 1; t <= S; ++t) {
        f4& hv = (u & 1) ? hB[t - 1] : hA[t - 1];
        const f4 old = hv;
        hv = nv;
        nv = axpy0(wp.v[u + S - t], old, wn.v[u + S - t], nv);
      }
      store(i, nv);
    }
  }
  vm_wait<0>();  // no LDS-DMA may land after the wave's LDS is released
}

template <int S, int D, int PF, bool SYNC = false>
__global__ __launch_bounds__(kThreads) void ring_stream_dma_kernel(
    const float* __restrict__ X, int64_t ldx, float* __restrict__ Y, int64_t ldy, int n_rows,
    int64_t ncols_v, uint32_t n_col_tiles, const float* __restrict__ wprev,
    const float* __restrict__ wnext, uint32_t n_row_tiles, int T, int order) {
  __shared__ __attribute__((aligned(16))) float lds[kThreads / 64][D][256];
  const uint32_t b = blockIdx.x;
  uint32_t ct;
  int r0;
  if (order == 0) {  // XCD-aware: an XCD walks its column tiles' row tiles in order (halo rows from L2)
    const uint32_t x = b & 7u, l = b >> 3;
    ct = (l / n_row_tiles) * 8 + x;
    r0 = static_cast<int>(l % n_row_tiles) * T;
  } else {  // column tile fastest: the chip sweeps row bands, as ring_mix_dma_kernel does
    const uint32_t nct8 = (n_col_tiles + 7) / 8 * 8;
    ct = b % nct8;
    r0 = static_cast<int>(b / nct8) * T;
  }
  if (ct >= n_col_tiles) return;  // the whole block
  int64_t c = int64_t(ct) * kThreads + threadIdx.x;
  const bool live = c < ncols_v;
  if (!SYNC && !live) return;
  if (!live) c = ncols_v - 1;  // SYNC: every wave reaches the barriers; a dead lane loads a valid column, stores nothing
  const int nT = min(T, n_rows - r0);
  float* ring = &lds[threadIdx.x >> 6][0][0];
  if (r0 - 2 * S >= 0 && r0 + nT + S + PF <= n_rows)  // every row and weight index in range
    ring_stream_dma_body<S, D, PF, true, SYNC>(X, ldx, Y, ldy, c, n_rows, r0, nT, wprev, wnext, ring, live);
  else
    ring_stream_dma_body<S, D, PF, false, SYNC>(X, ldx, Y, ldy, c, n_rows, r0, nT, wprev, wnext, ring, live);
}

template <typename V, class Epi = NoEpi>
void launch_ring(const float* X, int64_t ldx, float* Y, int64_t ldy, int n_rows, int64_t c_off,
                 int64_t ncols_v, int rpb, const float* hp, const float* hn, const float* wp,
                 const float* wn, hipStream_t s, const Epi& epi = Epi{}) {
  const int64_t n_col_tiles = cdiv(ncols_v, kThreads);
  const int64_t n_rg = cdiv(n_rows, rpb);
  const int64_t grid = n_col_tiles * n_rg;
  hipLaunchKernelGGL((ring_mix_kernel<V, Epi>), dim3(static_cast<unsigned>(grid)), dim3(kThreads), 0, s,
                     X, ldx, Y, ldy, n_rows, c_off, ncols_v, n_col_tiles, rpb, hp, hn, wp, wn, epi);
}

template <class Epi>
int mix_ring_impl(const char* nm, const float* X, int64_t ldx, float* Y, int64_t ldy, int32_t n_rows, int64_t P,
                  const float* halo_prev, const float* halo_next, const float* w_prev, const float* w_next,
                  const Epi& epi, bool epi_vec_ok, hipStream_t s) {
  DOL_CHECKED(check_rows(nm, n_rows < 0 || P < 0, n_rows == 0 || P == 0, !X || !Y || !w_prev || !w_next,
                         ldx < P || ldy < P, X == Y, kJacobiAlias));
  if ((halo_prev == nullptr) != (halo_next == nullptr)) return fail(DOL_EINVAL, "%s: pass both halos or neither", nm);
  if (!halo_prev) {
    if (n_rows < 3) return fail(DOL_EINVAL, "%s: wrap-around ring needs n_rows >= 3", nm);
    halo_prev = X + int64_t(n_rows - 1) * ldx;
    halo_next = X;
  }
  const bool vec_ok = row_vec_ok(X, ldx) && row_vec_ok(Y, ldy) && aligned16(halo_prev) && aligned16(halo_next) &&
                      epi_vec_ok;
  const ColSplit cs = split_cols(P, vec_ok);
  if (cs.n4 > 0) {
    constexpr int R = 4;
    const int64_t nct = cdiv(cs.n4, kThreads);
    if (mul_sat(nct, cdiv(n_rows, R)) > kMaxBlocks) return fail(DOL_EINVAL, "%s: problem too large for one launch", nm);
    hipLaunchKernelGGL((ring_mix_dma_kernel<R, Epi, true, false>), dim3(static_cast<unsigned>(nct * cdiv(n_rows, R))),
                       dim3(kThreads), 0, s, X, ldx, Y, ldy, n_rows, cs.n4, nct, halo_prev, halo_next, w_prev, w_next, epi);
  }
  if (cs.tail > 0) {
    if (mul_sat(cdiv(cs.tail, kThreads), cdiv(n_rows, kRingTailRows)) > kMaxBlocks)
      return fail(DOL_EINVAL, "%s: problem too large for one launch", nm);
    launch_ring<float, Epi>(X, ldx, Y, ldy, n_rows, cs.n4 * 4, cs.tail, kRingTailRows, halo_prev, halo_next, w_prev,
                            w_next, s, epi);
  }
  return check_launch(nm);
}

template <class Epi>
int ring_edges_impl(const char* nm, const float* X, int64_t ldx, float* Y, int64_t ldy, int32_t n_rows, int64_t P,
                    const float* halo_prev, const float* halo_next, const float* w_prev, const float* w_next,
                    const Epi& epi, bool epi_vec_ok, hipStream_t s) {
  DOL_CHECKED(check_rows(nm, n_rows < 0 || P < 0, n_rows == 0 || P == 0,
                         !X || !Y || !w_prev || !w_next || !halo_prev || !halo_next, ldx < P || ldy < P, X == Y,
                         kJacobiAlias));
  const bool vec_ok = row_vec_ok(X, ldx) && row_vec_ok(Y, ldy) && aligned16(halo_prev) && aligned16(halo_next) &&
                      epi_vec_ok;
  const ColSplit cs = split_cols(P, vec_ok);
  const unsigned ny = n_rows == 1 ? 1u : 2u;
  if (cs.n4 > 0)
    hipLaunchKernelGGL((ring_edges_kernel<f4, Epi>), dim3(static_cast<unsigned>(cdiv(cs.n4, kThreads)), ny),
                       dim3(kThreads), 0, s, X, ldx, Y, ldy, n_rows, int64_t(0), cs.n4, halo_prev, halo_next, w_prev,
                       w_next, epi);
  if (cs.tail > 0)
    hipLaunchKernelGGL((ring_edges_kernel<float, Epi>), dim3(static_cast<unsigned>(cdiv(cs.tail, kThreads)), ny),
                       dim3(kThreads), 0, s, X, ldx, Y, ldy, n_rows, cs.n4 * 4, cs.tail, halo_prev, halo_next, w_prev,
                       w_next, epi);
  return check_launch(nm);
}

}  // namespace

extern "C" {

int dol_mix_ring_f32(const float* X, int64_t ldx, float* Y, int64_t ldy, int32_t n_rows, int64_t P,
                     const float* halo_prev, const float* halo_next, const float* w_prev,
                     const float* w_next, hipStream_t s) {
  DOL_DIMS_OK("dol_mix_ring_f32", ldx, ldy, P);
  return mix_ring_impl("dol_mix_ring_f32", X, ldx, Y, ldy, n_rows, P, halo_prev, halo_next, w_prev, w_next,
                       NoEpi{}, true, s);
}

int dol_mix_ring_edges_f32(const float* X, int64_t ldx, float* Y, int64_t ldy, int32_t n_rows, int64_t P,
                           const float* halo_prev, const float* halo_next, const float* w_prev,
                           const float* w_next, hipStream_t s) {
  DOL_DIMS_OK("dol_mix_ring_edges_f32", ldx, ldy, P);
  return ring_edges_impl("dol_mix_ring_edges_f32", X, ldx, Y, ldy, n_rows, P, halo_prev, halo_next, w_prev, w_next,
                         NoEpi{}, true, s);
}

int dol_dgd_ring_f32(const float* X, int64_t ldx, float* Y, int64_t ldy, int32_t n_rows, int64_t P,
                     const float* halo_prev, const float* halo_next, const float* w_prev, const float* w_next,
                     const float* target, int64_t ldt, float* mom, int64_t ldm, int32_t objective,
                     int32_t local_steps, float lr, float momentum, int first_step, hipStream_t s) {
  DOL_DIMS_OK("dol_dgd_ring_f32", ldx, ldy, P, ldt, ldm);
  const char* nm = "dol_dgd_ring_f32";
  const DgdArgs d{target, ldt, mom, ldm, objective, local_steps, lr, momentum, first_step};
  return with_dgd_epi(nm, d, n_rows <= 0 || P <= 0, P, [&](auto epi, bool evec) {
    return mix_ring_impl(nm, X, ldx, Y, ldy, n_rows, P, halo_prev, halo_next, w_prev, w_next, epi, evec, s);
  });
}

int dol_dgd_ring_edges_f32(const float* X, int64_t ldx, float* Y, int64_t ldy, int32_t n_rows, int64_t P,
                           const float* halo_prev, const float* halo_next, const float* w_prev, const float* w_next,
                           const float* target, int64_t ldt, float* mom, int64_t ldm, int32_t objective,
                           int32_t local_steps, float lr, float momentum, int first_step, hipStream_t s) {
  DOL_DIMS_OK("dol_dgd_ring_edges_f32", ldx, ldy, P, ldt, ldm);
  const char* nm = "dol_dgd_ring_edges_f32";
  const DgdArgs d{target, ldt, mom, ldm, objective, local_steps, lr, momentum, first_step};
  return with_dgd_epi(nm, d, n_rows <= 0 || P <= 0, P, [&](auto epi, bool evec) {
    return ring_edges_impl(nm, X, ldx, Y, ldy, n_rows, P, halo_prev, halo_next, w_prev, w_next, epi, evec, s);
  });
}

// the EXTRA round (ExtraEpi, dol_launch.h) on the ring, wrap-around or with halos, and its two boundary rows
int dol_extra_ring_f32(const float* X, int64_t ldx, float* Y, int64_t ldy, int32_t n_rows, int64_t P,
                       const float* halo_prev, const float* halo_next, const float* w_prev, const float* w_next,
                       const float* w_self, const float* target, int64_t ldt, float* corr, int64_t ldc,
                       int32_t objective, float lr, hipStream_t s) {
  DOL_DIMS_OK("dol_extra_ring_f32", ldx, ldy, P, ldt, ldc);
  const char* nm = "dol_extra_ring_f32";
  const ExtraArgs e{target, ldt, corr, ldc, w_self, objective, lr};
  return with_extra_epi<true>(nm, e, X, ldx, Y, n_rows <= 0 || P <= 0, P, [&](auto epi, bool evec) {
    return mix_ring_impl(nm, X, ldx, Y, ldy, n_rows, P, halo_prev, halo_next, w_prev, w_next, epi, evec, s);
  });
}

int dol_extra_ring_edges_f32(const float* X, int64_t ldx, float* Y, int64_t ldy, int32_t n_rows, int64_t P,
                             const float* halo_prev, const float* halo_next, const float* w_prev,
                             const float* w_next, const float* w_self, const float* target, int64_t ldt, float* corr,
                             int64_t ldc, int32_t objective, float lr, hipStream_t s) {
  DOL_DIMS_OK("dol_extra_ring_edges_f32", ldx, ldy, P, ldt, ldc);
  const char* nm = "dol_extra_ring_edges_f32";
  const ExtraArgs e{target, ldt, corr, ldc, w_self, objective, lr};
  return with_extra_epi<false>(nm, e, X, ldx, Y, n_rows <= 0 || P <= 0, P, [&](auto epi, bool evec) {
    return ring_edges_impl(nm, X, ldx, Y, ldy, n_rows, P, halo_prev, halo_next, w_prev, w_next, epi, evec, s);
  });
}

// kernel of dol_mix_ring_steps_f32 chosen by dol_ring_steps_set_variant (0:
// the register tiles); atomic, so a setter on one thread never tears a launch's
// read on another (dol_mix_ring_steps_ex_f32 takes the variant per call)
static std::atomic<int> g_ring_steps_variant{0};

int dol_ring_steps_set_variant(int32_t variant) {
  if (variant < 0 || variant > kRingStepsVariants)
    return fail(DOL_EINVAL, "dol_ring_steps_set_variant: variant %d outside 0 (default) / 1 (tiles) / 2 (stream) / 3-5 (LDS-DMA stream: plain, synchronised, sweep)", variant);
  const int prev = g_ring_steps_variant.exchange(variant, std::memory_order_relaxed);
  g_err[0] = '\0';
  return prev;
}

int dol_mix_ring_steps_f32(const float* X, int64_t ldx, float* Y, int64_t ldy, int32_t n_rows,
                           int64_t P, int32_t steps, const float* w_prev, const float* w_next,
                           hipStream_t s) {
  return dol_mix_ring_steps_ex_f32(X, ldx, Y, ldy, n_rows, P, steps, w_prev, w_next, 0, s);
}

int dol_mix_ring_steps_ex_f32(const float* X, int64_t ldx, float* Y, int64_t ldy, int32_t n_rows,
                              int64_t P, int32_t steps, const float* w_prev, const float* w_next,
                              int32_t variant, hipStream_t s) {
  DOL_DIMS_OK("dol_mix_ring_steps_f32", ldx, ldy, P);
  if (variant < 0 || variant > kRingStepsVariants)
    return fail(DOL_EINVAL, "dol_mix_ring_steps_ex_f32: variant %d outside 0 (process setting) / 1 (tiles) / 2 (stream) / 3-5 (LDS-DMA stream: plain, synchronised, sweep)", variant);
  DOL_CHECKED(check_rows("dol_mix_ring_steps_f32", n_rows < 0 || P < 0 || steps < 0, n_rows == 0 || P == 0,
                         !X || !Y || !w_prev || !w_next, ldx < P || ldy < P, X == Y));
  if (n_rows < 3) return fail(DOL_EINVAL, "dol_mix_ring_steps_f32: a ring needs n_rows >= 3");
  if (steps == 0) return fail(DOL_EINVAL, "dol_mix_ring_steps_f32: steps must be >= 1");
  const bool vec = row_vec_ok(X, ldx) && row_vec_ok(Y, ldy) && P % 4 == 0;
  if (!vec || steps > 8) return fail(DOL_EINVAL, "dol_mix_ring_steps_f32: needs 16-B aligned rows, P %% 4 == 0 and steps <= 8 (compose launches otherwise)");
  // Five kernels give the same bits; the variant picks one: 1 ring_steps_kernel
  // (register tiles), 2 ring_stream_kernel (1024-row tiles, 8 rows in flight,
  // nontemporal loads), 3 / 4 / 5 ring_stream_dma_kernel (plain / block-
  // synchronised / column-tile-fastest sweep of 64-row tiles).  Variant 0 is
  // the process setting (dol_ring_steps_set_variant), else the register tiles.
  // eps = 5 at 8192 x 2^20, alternating on one box (profiles/r03_eps_stream.txt):
  // box A stream 12.38 / 12.39 vs tiles 12.61 / 12.62 ms; box C stream-NT 11.60 /
  // 12.00 / 11.76 vs tiles 11.90 / 11.92 / 11.80; box E stream-NT 12.95-13.19 vs
  // tiles 11.96-12.67; the stream kernel alone ran 10.66 ms on one box and 12.72
  // on another with the same ring round (10.92 ms): no consistent winner, so the
  // r02 default stays.  Clock 1 % below the ring kernel's for both (2424 / 2408
  // vs 2439 MHz, GRBM_GUI_ACTIVE per XCD over the kernel's time).
  // Which variant wins follows where the bank's pages landed, as for the
  // parameter-major mix (profiles/r03_pm_stage_order.txt): ops.tune_ring_steps_variant
  // times them on the buffers in use and keeps the fastest (dol_ring_steps_set_variant).
  const int v = variant != 0 ? variant : g_ring_steps_variant.load(std::memory_order_relaxed);
  const bool stream = v >= 2;
  auto go_stream = [&](auto steps_c) {
    constexpr int S = decltype(steps_c)::value;
    const int T = v == 5 ? 64 : 1024;  // tile rows
    const int64_t nv = P / 4;
    const uint32_t nct = static_cast<uint32_t>(cdiv(nv, kThreads));
    const int64_t nrt = cdiv(n_rows, T);
    const int64_t grid = cdiv(nct, 8) * 8 * nrt;
    if (grid > kMaxBlocks) return fail(DOL_EINVAL, "dol_mix_ring_steps_f32: too large");
    const dim3 g(static_cast<unsigned>(grid)), b(kThreads);
    const uint32_t nrt32 = static_cast<uint32_t>(nrt);
    const int order = v == 5 ? 1 : 0;  // 0 = XCD-aware row-tile order, 1 = column tile fastest (sweep)
    if (v == 2)
      hipLaunchKernelGGL((ring_stream_kernel<S, 8>), g, b, 0, s, X, ldx, Y, ldy, n_rows, nv, nct, w_prev, w_next, nrt32, T);
    else if (v == 4)  // one raw barrier per 8 steps keeps a block's waves on the same rows
      hipLaunchKernelGGL((ring_stream_dma_kernel<S, 8, 8, true>), g, b, 0, s, X, ldx, Y, ldy, n_rows, nv, nct, w_prev,
                         w_next, nrt32, T, order);
    else  // 8-row LDS-DMA ring per wave
      hipLaunchKernelGGL((ring_stream_dma_kernel<S, 8, 8>), g, b, 0, s, X, ldx, Y, ldy, n_rows, nv, nct, w_prev, w_next,
                         nrt32, T, order);
    return check_launch("dol_mix_ring_steps_f32");
  };

  // tile heights R by S, measured at 8192 x 2^20 (tools/bench_configs.py ring-eps<S>):
  // R = 6 for S <= 3 (4 for S = 1), 14 for S = 4, 22 for S = 5-6, 30 for S = 7-8
  static constexpr int kTileRows[9] = {0, 4, 6, 6, 14, 22, 22, 30, 30};
  return dispatch([&](auto steps_c) {
    constexpr int S = decltype(steps_c)::value, R = kTileRows[S];
    // the stream kernels wrap at most once, so smaller rings take the register
    // tiles; the LDS-DMA one's buffer stores address a row in 32 bits
    if (stream && n_rows >= 2 * S + 16 + 1 && (v < 3 || ldy * 4 < (int64_t(1) << 31))) return go_stream(steps_c);
    using V = f4;
    const int64_t nv = P / Vec<V>::W;
    const uint32_t nct = static_cast<uint32_t>(cdiv(nv, kThreads));
    const int64_t nrt = cdiv(n_rows, R);
    const int64_t grid = cdiv(nct, 8) * 8 * nrt;
    if (grid > kMaxBlocks) return fail(DOL_EINVAL, "dol_mix_ring_steps_f32: too large");
    hipLaunchKernelGGL((ring_steps_kernel<S, R, V>), dim3(static_cast<unsigned>(grid)), dim3(kThreads), 0, s, X, ldx, Y,
                       ldy, n_rows, nv, nct, w_prev, w_next, static_cast<uint32_t>(nrt));
    return check_launch("dol_mix_ring_steps_f32");
  }, Ints<1, 2, 3, 4, 5, 6, 7, 8>{steps});
}

int dol_stream_copy_rows_f32(const float* X, int64_t ldx, float* Y, int64_t ldy, int32_t n_rows, int64_t P,
                             hipStream_t s) {
  DOL_DIMS_OK("dol_stream_copy_rows_f32", ldx, ldy, P);
  const char* nm = "dol_stream_copy_rows_f32";
  DOL_CHECKED(check_rows(nm, n_rows < 0 || P < 0, n_rows == 0 || P == 0, !X || !Y, ldx < P || ldy < P, false));
  if (n_rows < 3 || !row_vec_ok(X, ldx) || !row_vec_ok(Y, ldy) || P % 4)
    return fail(DOL_EINVAL, "%s: needs >= 3 rows, 16-B aligned rows and P %% 4 == 0", nm);
  constexpr int R = 4;
  const int64_t n4 = P / 4, nct = cdiv(n4, kThreads);
  if (mul_sat(nct, cdiv(n_rows, R)) > kMaxBlocks) return fail(DOL_EINVAL, "%s: too large", nm);
  // the ring mix's launch with COPY: halo rows = the wrap-around neighbours, weights unused
  const float* hp = X + int64_t(n_rows - 1) * ldx;
  hipLaunchKernelGGL((ring_mix_dma_kernel<R, NoEpi, true, true>), dim3(static_cast<unsigned>(nct * cdiv(n_rows, R))),
                     dim3(kThreads), 0, s, X, ldx, Y, ldy, n_rows, n4, nct, hp, X, X, X, NoEpi{});
  return check_launch(nm);
}

}  // extern "C"
