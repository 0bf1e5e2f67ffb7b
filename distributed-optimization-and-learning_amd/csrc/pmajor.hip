// pmajor.hip — the sparse gossip mix on the PARAMETER-MAJOR ("transposed")
// bank layout, and the layout conversion.  Part of libdol_hip.so.
//
// Layout.  The agent-major bank (row k = agent k's P parameters, ring.hip / csr.hip)
// is what the notebooks' nn.Module views need.  For synthetic many-agent
// workloads whose local steps are per coordinate (BASELINE config 3: 1024-8192
// agents x 2^20 on a random-regular W) the engine can hold the bank
// transposed instead: XT[p][j] = agent j's parameter p, p-row stride ldx >= N.
// One p-row is then the whole mixing problem for one coordinate,
// Y[:, p] = W X[:, p], and it is CONTIGUOUS (N floats: 4 KiB at 1024 agents,
// 32 KiB at 8192): every byte of X and Y streams once, sequentially, whatever
// the graph — where the agent-major CSR kernel re-reads each row deg times
// through L2 (47-53 % of HBM on random-regular W).
//
// csr_pm_kernel: one persistent 1024-thread workgroup per CU walks 32 KiB
// stages (sr consecutive p-rows, each padded to xw floats in LDS); stages come
// in by LDS-DMA (global_load_lds_dwordx4) into a ring of NBUF buffers with
// NBUF - 1 stages in flight, retired by a counted s_waitcnt vmcnt and a raw
// s_barrier (no __syncthreads(): its fence would drain the ring).  Each thread
// owns QPT "quads" (4 consecutive output agents) for the whole kernel, with
// their first four (column, weight) pairs in registers (columns as u16), so the
// CSR index is read once per kernel, not once per tile; the gathers are LDS
// reads.  Sums: +0 start, ascending CSR order, separately rounded mul and add
// (-ffp-contract=off), entries past a row's degree skipped by a select (no
// 0 * Inf) — bit-identical to dol_mix_csr_f32 and the reference's consensus
// (DIST/clients.py:61-69).  Stores are buffer stores with dropped
// out-of-range lanes, so every thread issues the same number of VMEM ops per
// stage and the counted wait is exact.
//
// csr_pm_steps_kernel: the same pipeline with eps >= 2 mixing steps per stage
// (FedLCon's X <- W^eps X, DIST/simulators.py:190-196).  Steps 2 .. eps of a
// coordinate need only its p-row, which is whole in LDS, so they run LDS to
// LDS between the stage image and one scratch image and the bank still
// crosses HBM once.  Geometry: up to 4096 agents 48 KiB x 2 + <= 48 KiB
// scratch (the mix and all modes of the fused round); beyond, 32 KiB x 4 +
// 32 KiB (all 160 KiB; the ring drops from five buffers to four).  Measured,
// random 4-regular W, (a) eps single-step launches against (b) the fused pass
// in one process on the same buffers (tools/pm_steps_ab.py,
// profiles/pm_steps_ab.jsonl); HBM = 2 N P 4 bytes over (b) at 8 TB/s:
//   1024 x 2^20  eps 2 / 3 / 5 / 8: (a) 3.29 / 4.94 / 8.22 / 13.15 ms,
//                (b) 2.14 / 3.09 / 4.99 / 7.85 ms, (b)/(a) 0.65 / 0.62 / 0.61 / 0.60,
//                HBM 50 / 35 / 22 / 14 %
//   8192 x 2^20  (a) 24.26 / 35.90 / 60.13 / 96.83, (b) 19.91 / 27.74 / 43.41 / 66.98,
//                (b)/(a) 0.82 / 0.77 / 0.72 / 0.69, HBM 43 / 31 / 20 / 13 %
// An extra step is 0.95 ms at 1024 agents (LDS-bound: random-bank conflicts
// and two barriers per step) and 7.8 ms at 8192.  Alternatives up to 4096
// agents, eps 2 / 5 at 1024 x 2^20 (profiles/pm_steps_geom.txt): 48 KiB x 2 +
// 48 KiB 2.15 / 5.01 ms; 64 KiB x 2 + 32 KiB scratch (sr cut to fit it) 2.37 /
// 5.32; 32 KiB x 3 + 32 KiB 2.32 / 5.29 -- more p-rows per barrier won.  The
// fused round, eps 5, 1024 x 2^20: least squares + momentum 6.73 ms against
// 10.00 for four mixes and the round, logistic 6.73 against 8.74.
//
// csr_pm_gt_kernel: config 3's gradient-tracking round (x' = W x - lr s,
// s' = W s + g(x') - g(x)) in the same pipeline.  A stage holds X, S and T
// images; X and S are gathered through the same Quad, the own x, s, t are f4
// LDS reads, g is recomputed: 5 N P 4 bytes per round.  91 (least squares) /
// 89 (logistic) VGPRs, no scratch (hipcc's resource remarks); built on
// issue_stage it took 128 VGPRs and 20-28 B of scratch at 80 KiB stages, hence
// its own packed stage issue.  Geometry, rr4 + Metropolis self weights, least
// squares / logistic ms at 1024 x 2^20 (4096 x 2^18), profiles/gt_pm_geom.jsonl:
//   80 KiB x 2  3.88 / 4.71 (3.67 / 4.65)     <- least squares
//   64 KiB x 2  4.17 / 4.47 (4.17 / 4.46)
//   48 KiB x 3  4.23 / 4.42 (4.23 / 4.43)     <- logistic
// Legs (tools/gt_ab.py, profiles/gt_pm_ab.jsonl; one process, same buffers,
// medians of 5 windows): (a) the round composed from two mixes, two gradient
// passes and the elementwise ops, (b) this kernel, (c) the least-squares +
// momentum DGD round above (the same five streams); HBM = 5 N P 4 bytes over
// (b) at 8 TB/s:
//   1024 x 2^20  least squares (a) 20.46 (b) 4.13 (c) 3.82 ms, (b)/(a) 0.20, (b)/(c) 1.08, HBM 65 %
//                logistic      (a) 20.42 (b) 4.22 (c) 3.82,    0.21, 1.11, 64 %
//   4096 x 2^18  least squares (a) 20.52 (b) 3.53 (c) 3.83,    0.17, 0.92, 76 %
//                logistic      (a) 20.49 (b) 4.24 (c) 3.83,    0.21, 1.11, 63 %
// (b) moved between 3.64 and 3.98 ms from process to process.  The S gather
// replaced by the own-element read (a build for that measurement only,
// profiles/gt_pm_probe.jsonl): least squares 3.92-3.98 ms, no gain; logistic
// 3.99-4.03 against 4.24-4.27.  Counters per launch at 1024 x 2^20
// (profiles/gt_pm_counters.json): FETCH_SIZE 6 291 733 KiB (x 2: 1.00004 x the
// 3 N P 4 read), WRITE_SIZE 8 389 153 KiB (1.00006 x the 2 N P 4 written).
//
// csr_pm_extra_kernel: config 3's EXTRA round (x' = W x - lr g(x) - c, c' = c +
// (x - W x) / 2, extra_finish of dol_launch.h) in the same pipeline.  Only X is
// gathered, so a stage is the DGD round's mode-2 stage with the correction in
// the momentum's place: X, T and C images; the own x, t, c are f4 LDS reads;
// X' goes to YT and c' back to C in place, after the barrier that retires the
// stage's DMA (a C p-row belongs to one workgroup): 5 N P 4 bytes per round.
// csr_pm_gt_kernel's packed stage issue; 81 (least squares) / 87 (logistic)
// VGPRs, no scratch (hipcc's resource remarks; 85 / 91 at 80 KiB x 2, 81 / 87 at
// 64 KiB x 2, no scratch either).  Geometry, rr4 + Metropolis self weights, a
// build that took the geometry per call, one process, same buffers, medians of
// 5 alternating windows, least squares / logistic ms at 1024 x 2^20 (4096 x
// 2^18), window spread 0.1-0.6 %, profiles/extra_pm_geom.jsonl:
//   80 KiB x 2  4.33 / 4.35 (3.42 / 3.67)
//   64 KiB x 2  4.22 / 4.23 (3.41 / 3.51)
//   48 KiB x 3  4.09 / 4.15 (3.45 / 3.56)     <- both objectives
// 48 KiB x 3 beats 80 KiB x 2 by 5.4 / 4.7 % at 1024 agents and by 3.1 % for
// logistic at 4096; at 4096 agents (one p-row per stage in every geometry)
// least squares is 0.7 % behind 80 KiB x 2 and logistic 1.2 % behind 64 KiB x 2.
// Legs (tools/extra_ab.py --layout pm, profiles/extra_pm_ab.jsonl; another box,
// one process, same buffers, medians of 5 windows): (a) this kernel, (b)
// csr_pm_gt_kernel, (c) the least-squares / logistic + momentum DGD round (the
// same five streams), (d) ops.extra_csr on the same problem agent-major (equal
// bit for bit); HBM = 5 N P 4 bytes over (a) at 8 TB/s:
//   1024 x 2^20  least squares (a) 3.86 (b) 3.95 (c) 3.90 (d) 4.98 ms, (a)/(c) 0.990, (a)/(d) 0.775, HBM 70 %
//                logistic      (a) 3.87 (b) 4.36 (c) 3.84 (d) 4.97,    1.007, 0.779, 69 %
//   4096 x 2^18  least squares (a) 4.14 (b) 3.60 (c) 4.02 (d) 4.89,    1.031, 0.847, 65 %
//                logistic      (a) 4.12 (b) 4.39 (c) 4.01 (d) 4.91,    1.029, 0.839, 65 %
// Counters per launch at 1024 x 2^20 (profiles/extra_pm_counters.json):
// FETCH_SIZE x 2 1.00004 x the 3 N P 4 read, WRITE_SIZE 1.0004 x / 1.00009 x the
// 2 N P 4 written.
//
// Tried and retired (each was a launch variant behind an environment switch;
// the code last existed in commit 2d96633):
//  * DOL_PM_DGD_GEOM, the fused round's stage geometry forced to 64 KiB x 2,
//    48 KiB x 3 or 80 KiB x 2: at 1024 x 2^20 rr4, least squares + momentum
//    3.45 ms on 80 KiB x 2 vs 3.56 (64 KiB x 2) and 3.49 (48 KiB x 3);
//    logistic, no momentum, 2.25 on 64 KiB x 2 vs 2.43 / 2.55.  Each mode now
//    has the geometry that won: 80 KiB x 2 with the momentum read (mode 2),
//    64 KiB x 2 without.
//  * DOL_PM_BIG_NB=4, four 32-KiB buffers beyond 4096 agents (r01); five won
//    (profiles/r02_pm_nbuf.txt).
//  * DOL_PM_VARIANT 1 / 4, the plain mix with default-policy (not
//    nontemporal) LDS-DMA loads, and a copy y = x in the same geometry (the
//    structure's own ceiling): measurement only.
#include <algorithm>
#include <atomic>

#include "dol_launch.h"

namespace {
constexpr int kMaxAgents = 8192;          // one p-row image fits a 32 KiB stage
constexpr int kT1 = 1024;                 // threads per workgroup (16 waves, one workgroup per CU)
constexpr int kNT = 2;                    // cache-policy bits of the LDS-DMA loads and the stores: nontemporal

__device__ __forceinline__ void wait_vmcnt(int n) {
  switch (n) {
#define DOL_VMC(N) case N: asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory"); break;
#define DOL_VMC8(N) DOL_VMC(N) DOL_VMC(N + 1) DOL_VMC(N + 2) DOL_VMC(N + 3) DOL_VMC(N + 4) DOL_VMC(N + 5) DOL_VMC(N + 6) DOL_VMC(N + 7)
    DOL_VMC(1) DOL_VMC(2) DOL_VMC(3) DOL_VMC(4) DOL_VMC(5) DOL_VMC(6) DOL_VMC(7)
    DOL_VMC8(8) DOL_VMC8(16) DOL_VMC8(24) DOL_VMC8(32) DOL_VMC8(40) DOL_VMC8(48) DOL_VMC8(56)
#undef DOL_VMC8
#undef DOL_VMC
    default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
  }
}

__device__ __forceinline__ rsrc_t make_rsrc(const float* p, uint32_t nbytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p), 0, static_cast<int>(nbytes), 0x00020000);
}

// one output quad: agents 4q .. 4q+3, their first four neighbours (u16 columns,
// two per register), weights and degrees (4 bits each, min(degree, 15))
struct Quad {
  uint32_t c[4][2];
  float w[4][4];
  uint32_t deg;
};

__device__ __forceinline__ void load_quad(Quad& Q, int q, int n_rows, int nnz, const int32_t* __restrict__ rowptr,
                                          const int32_t* __restrict__ col, const float* __restrict__ val) {
  // unconditional loads from clamped addresses, all issued before any use (a
  // predicated load compiles to a branch + vmcnt(0) per element)
  int e0[4], d[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int i = min(4 * q + a, n_rows - 1);
    e0[a] = rowptr[i];
    d[a] = rowptr[i + 1];
  }
  int cj[4][4];
  float wj[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    d[a] = 4 * q + a < n_rows ? d[a] - e0[a] : 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int ee = min(e0[a] + e, nnz - 1);
      cj[a][e] = col[ee];
      wj[a][e] = val[ee];
    }
  }
  Q.deg = 0;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    Q.deg |= uint32_t(d[a] < 15 ? d[a] : 15) << (4 * a);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool in = e < d[a];
      const uint32_t c = in ? static_cast<uint32_t>(cj[a][e]) : 0u;
      if (e % 2 == 0) Q.c[a][e / 2] = c;
      else Q.c[a][e / 2] |= c << 16;
      Q.w[a][e] = in ? wj[a][e] : 0.0f;
    }
  }
}

// y[a] = sum_e w[a][e] * im[col[a][e]]  (+0 start, ascending e)
__device__ __forceinline__ f4 mix_quad(const Quad& Q, const float* __restrict__ im, int q,
                                       const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                       const float* __restrict__ val) {
  f4 y;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int d = static_cast<int>((Q.deg >> (4 * a)) & 15u);
    float acc = 0.0f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t cj = (Q.c[a][e / 2] >> (16 * (e % 2))) & 0xffffu;
      const float t = Q.w[a][e] * im[cj];
      acc = e < d ? acc + t : acc;
    }
    if (d > 4) {  // a long row: the rest of its list from memory (rare; correct, not fast)
      const int i = 4 * q + a;
      const int e1 = rowptr[i + 1];
      for (int e = rowptr[i] + 4; e < e1; ++e) acc = acc + val[e] * im[col[e]];
    }
    y[a] = acc;
  }
  return y;
}

// Config-3 epilogue on the parameter-major bank (the DGD round of
// dol_dgd_csr_f32, transposed): after the mix, `steps` local momentum-SGD
// iterations on the separable loss, per coordinate (OBJ 0 least squares
// g = x - t, 1 logistic g = -t / (1 + exp(t x)); MODE 0 plain SGD, 1 first
// momentum step, 2 momentum), x = fma(-lr, d, x) — dgd_local_steps of
// dol_launch.h, the arithmetic of DgdEpi / oracle_dgd_local_f32.  The target
// (and momentum) p-rows of a stage come in by the same LDS-DMA as X, behind
// the X image.
struct PmDgd {
  const float* T; int64_t ldt;
  float* M; int64_t ldm;
  float neg_lr, mom;
  int steps;
};

// Mix one stage image (sr p-rows of xw floats at im0, p-rows p0 ..) and store
// its rows of YT (and, OBJ >= 0, run the local steps first: target / momentum
// images of nw floats per p-row at tim0, behind the stage's X image as it came
// in -- which the multi-step kernel's im0 need not be): spt (x2 with a momentum
// store) buffer stores per thread, out-of-range ones dropped.
template <int T, int QPT, int OBJ = -1, int MODE = 0>
__device__ __forceinline__ void mix_stage(const Quad (&Q)[QPT], const float* __restrict__ im0, float* __restrict__ YT,
                                          int64_t ldy, int n_rows, int64_t P, int64_t p0, int xw, int sr, int spt,
                                          int q0, int g, int GR, const int32_t* __restrict__ rowptr,
                                          const int32_t* __restrict__ col, const float* __restrict__ val,
                                          const PmDgd& e, int nw, const float* __restrict__ tim0) {
  const int nq = (n_rows + 3) / 4;
  const int64_t rows_here = std::min<int64_t>(sr, P - p0);
  const rsrc_t ry = make_rsrc(YT + p0 * ldy, static_cast<uint32_t>(rows_here * ldy * 4));
  rsrc_t rm = ry;
  if constexpr (OBJ >= 0 && MODE != 0) rm = make_rsrc(e.M + p0 * e.ldm, static_cast<uint32_t>(rows_here * e.ldm * 4));
  const float* mim0 = tim0 + sr * nw;     // momentum images (MODE 2)
  for (int u = 0; u < spt / QPT; ++u) {
    const int pr = g + u * GR;
    const bool prow_ok = pr < rows_here;
    const int prc = pr < sr ? pr : 0;
    const float* im = im0 + prc * xw;
#pragma unroll
    for (int j = 0; j < QPT; ++j) {
      const int q = q0 + j * T;
      f4 y = mix_quad(Q[j], im, q, rowptr, col, val);
      f4 bv = f4{0.f, 0.f, 0.f, 0.f};
      if constexpr (OBJ >= 0) {
        const int qc = q < nq ? q : 0;
        const f4 tv = *reinterpret_cast<const f4*>(tim0 + prc * nw + 4 * qc);
        if constexpr (MODE == 2) bv = *reinterpret_cast<const f4*>(mim0 + prc * nw + 4 * qc);
        float b0 = bv.x, b1 = bv.y, b2 = bv.z, b3 = bv.w;
        y = f4{dgd_local_steps<OBJ, MODE>(y.x, tv.x, b0, e), dgd_local_steps<OBJ, MODE>(y.y, tv.y, b1, e),
               dgd_local_steps<OBJ, MODE>(y.z, tv.z, b2, e), dgd_local_steps<OBJ, MODE>(y.w, tv.w, b3, e)};
        bv = f4{b0, b1, b2, b3};
      }
      const uint32_t off = static_cast<uint32_t>((pr * ldy + 4 * q) * 4);
      const uint32_t offm = static_cast<uint32_t>((pr * (OBJ >= 0 && MODE != 0 ? e.ldm : 0) + 4 * q) * 4);
      constexpr bool kMom = OBJ >= 0 && MODE != 0;
      if (4 * q + 3 < n_rows || q >= nq) {  // whole quad, or none (dropped)
        const bool ok = prow_ok && q < nq;
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4, y), ry, ok ? off : kOOB, 0, kNT);
        if constexpr (kMom)
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4, bv), rm, ok ? offm : kOOB, 0, kNT);
      } else {  // the ragged last quad (elements named one by one: hipcc 7.2 stored
                // element 0 four times from a loop over y[a] here)
        const float ye[4] = {y.x, y.y, y.z, y.w};
        const int left = n_rows - 4 * q;  // 1..3
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(ye[0]), ry, prow_ok ? off : kOOB, 0, kNT);
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(ye[1]), ry, prow_ok && left > 1 ? off + 4 : kOOB, 0,
                                              kNT);
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(ye[2]), ry, prow_ok && left > 2 ? off + 8 : kOOB, 0,
                                              kNT);
        if constexpr (kMom) {
          const float be[4] = {bv.x, bv.y, bv.z, bv.w};
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(be[0]), rm, prow_ok ? offm : kOOB, 0, kNT);
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(be[1]), rm, prow_ok && left > 1 ? offm + 4 : kOOB, 0,
                                                kNT);
          __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(be[2]), rm, prow_ok && left > 2 ? offm + 8 : kOOB, 0,
                                                kNT);
        }
      }
    }
  }
}

// One stage into the ring buffer at dst by LDS-DMA: the sr p-rows from p0 as
// nX 16-B pieces of X images (xq per p-row, the first xr4 holding data), then
// (OBJ >= 0) the target and (MODE 2) momentum images, nTM pieces each (nq4 per
// p-row, nr4 holding data).  SF / 4 / T loads per thread, dead pieces
// included, so the counted wait is the same for every thread.
template <int T, int SF, int OBJ, int MODE>
__device__ __forceinline__ void issue_stage(float* dst, const float* __restrict__ XT, int64_t ldx, int64_t P,
                                            int64_t p0, int xq, int xr4, int nq4, int nr4, int nX, int nTM,
                                            const PmDgd& e, int tid, int wave) {
#pragma unroll
  for (int d = 0; d < SF / 4 / T; ++d) {
    const int pc = d * T + tid;
    const float* src = XT;  // dead pieces re-read XT[0..3]
    if (pc < nX) {
      const int pr = pc / xq, j4 = pc - pr * xq;
      if (p0 + pr < P && j4 < xr4) src = XT + (p0 + pr) * ldx + 4 * j4;
    } else if (OBJ >= 0) {
      const int pt = pc - nX, op = pt / nTM, r = pt - op * nTM;  // op 0: target, 1: momentum
      const int pr = r / nq4, j4 = r - pr * nq4;
      if ((op == 0 || (MODE == 2 && op == 1)) && p0 + pr < P && j4 < nr4)
        src = op == 0 ? e.T + (p0 + pr) * e.ldt + 4 * j4 : e.M + (p0 + pr) * e.ldm + 4 * j4;
    }
    __builtin_amdgcn_global_load_lds(DOL_GPTR(src), DOL_LPTR(dst + (d * T + wave * 64) * 4), 16, 0, kNT);
  }
}

// T threads per workgroup, SF floats per stage buffer, NBUF buffers, QPT
// quads per thread.
// OBJ >= 0: the config-3 epilogue (PmDgd), its target (+ momentum) p-rows
// staged behind X's in every stage (nw floats each).
template <int T, int SF, int NBUF, int QPT, int OBJ = -1, int MODE = 0>
__global__ __launch_bounds__(T) void csr_pm_kernel(const float* __restrict__ XT, int64_t ldx, int x_rows,
                                                   float* __restrict__ YT, int64_t ldy, int n_rows, int64_t P,
                                                   int xw, int sr, int qp_log2, int spt, int64_t n_stages, int nseg,
                                                   const int32_t* __restrict__ rowptr,
                                                   const int32_t* __restrict__ col,
                                                   const float* __restrict__ val, PmDgd e, int nw, int wait_all_stores) {
  constexpr int kDma = SF / 4 / T;  // LDS-DMA instructions per thread per stage
  static_assert(kDma * 4 * T == SF, "a stage is a whole number of DMA rounds");
  extern __shared__ __attribute__((aligned(16))) float img[];  // NBUF x SF
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // thread -> (quad, p-row group): QPT == 1: QP = 2^qp_log2 quads per p-row,
  // GR = T / QP p-rows side by side; QPT > 1: quads tid + j*T of one p-row
  const int q0 = QPT == 1 ? (tid & ((1 << qp_log2) - 1)) : tid;
  const int g = QPT == 1 ? (tid >> qp_log2) : 0;
  const int GR = QPT == 1 ? (T >> qp_log2) : 1;
  const int nnz = rowptr[n_rows];
  Quad Q[QPT];
  if (nnz > 0) {
#pragma unroll
    for (int j = 0; j < QPT; ++j) load_quad(Q[j], q0 + j * T, n_rows, nnz, rowptr, col, val);
  } else {
#pragma unroll
    for (int j = 0; j < QPT; ++j) Q[j] = Quad{};
  }

  // stage order: the P range is cut into nseg contiguous segments; workgroup b
  // walks segment b % nseg with stride gridDim / nseg, so the chip streams
  // nseg separate regions at once (nseg = 8: +4-5 % over one sweep)
  const int64_t W = gridDim.x / nseg, seg = blockIdx.x % nseg, wl = blockIdx.x / nseg;
  const int64_t seg_len = (n_stages + nseg - 1) / nseg;
  const int64_t seg_n = std::max<int64_t>(0, std::min<int64_t>(seg_len, n_stages - seg * seg_len));
  const int64_t nk = wl < seg_n ? (seg_n - wl + W - 1) / W : 0;
  auto stage_of = [&](int64_t k) { return seg * seg_len + wl + k * W; };
  const int xq = xw / 4;             // 16-B pieces per p-row image
  const int xr4 = (x_rows + 3) / 4;  // pieces holding data
  const int nq4 = nw / 4, nr4 = (n_rows + 3) / 4;
  const int nX = sr * xq, nTM = sr * nq4;  // pieces of the X images, of one epilogue operand's images
  auto issue = [&](int64_t k) {      // stage k of this workgroup -> buffer k % NBUF
    issue_stage<T, SF, OBJ, MODE>(img + (k % NBUF) * SF, XT, ldx, P, stage_of(k) * sr, xq, xr4, nq4, nr4, nX, nTM, e,
                                  tid, wave);
  };
  constexpr int kStores = (OBJ >= 0 && MODE != 0) ? 2 : 1;  // buffer stores per (p-row, quad)
#pragma unroll
  for (int k = 0; k < NBUF - 1; ++k)
    if (k < nk) issue(k);
  for (int64_t k = 0; k < nk; ++k) {
    // retire stage k: the ops younger than its DMA are the stages issued after
    // it and the stores of every stage mixed since it was issued -- min(k,
    // NBUF - 1) of them (vmcnt retires loads and stores in issue order).  r04:
    // the count before held one stage's stores, so with NBUF > 2 each stage
    // also waited for the write acknowledgements of the stores NBUF - 2 stages
    // back (DOL_PM_WAIT=0 restores it, for measurement).
    const int64_t ahead = std::min<int64_t>(nk - 1, k + NBUF - 2) - k;
    const int64_t st_groups = wait_all_stores ? std::min<int64_t>(k, NBUF - 1) : (k >= 1 ? 1 : 0);
    wait_vmcnt(static_cast<int>(std::min<int64_t>(63, kStores * spt * st_groups + kDma * ahead)));
    __builtin_amdgcn_s_barrier();  // every wave's share landed; buffer (k-1) % NBUF is free
    if (k + NBUF - 1 < nk) issue(k + NBUF - 1);
    const int64_t p0 = stage_of(k) * sr;
    const float* im0 = img + (k % NBUF) * SF;
    mix_stage<T, QPT, OBJ, MODE>(Q, im0, YT, ldy, n_rows, P, p0, xw, sr, spt, q0, g, GR, rowptr, col, val, e, nw,
                                 im0 + sr * xw);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this stage's LDS reads are done before the next barrier
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// One intermediate mixing step of a stage, LDS to LDS: the image at dst gets
// W times the image at src for the stage's live p-rows (same layout, xw
// floats per p-row), every thread writing the quads it owns as one 16-B LDS
// store.  The ragged last quad writes its dead lanes (+0) too: they lie below
// 4 * ceil(n / 4) <= xw and no gather reads them (col < n).  No vector-memory
// operation except a long row's fallback loads, which mix_quad consumes at
// once -- nothing is left in flight for the caller's counted wait.
template <int T, int QPT>
__device__ __forceinline__ void mix_image(const Quad (&Q)[QPT], const float* src, float* dst, int n_rows, int rows_here,
                                          int xw, int spt, int q0, int g, int GR,
                                          const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                          const float* __restrict__ val) {
  const int nq = (n_rows + 3) / 4;
  for (int u = 0; u < spt / QPT; ++u) {
    const int pr = g + u * GR;
    if (pr >= rows_here) continue;
#pragma unroll
    for (int j = 0; j < QPT; ++j) {
      const int q = q0 + j * T;
      if (q < nq) *reinterpret_cast<f4*>(dst + pr * xw + 4 * q) = mix_quad(Q[j], src + pr * xw, q, rowptr, col, val);
    }
  }
}

// csr_pm_kernel with mix_steps >= 2 mixing steps per stage (X <- W^k X, the
// inner loop of FedLCon's round, DIST/simulators.py:190-196): a stage's p-rows
// are complete in LDS, and step t + 1 of a coordinate needs nothing but step
// t's p-row, so the bank still crosses HBM once.  Stage image A (ring buffer
// k % NBUF) is mixed into one scratch image S behind the ring, S back into A,
// and so on; the last step mixes from whichever holds step mix_steps - 1 and
// stores from registers as mix_stage always does (the epilogue operands stay
// where the DMA put them, behind A's X part).  Between steps: s_waitcnt
// lgkmcnt(0) and a raw s_barrier, which order LDS against LDS only -- the
// intermediate steps issue no vector-memory operation, so the ring's vmcnt
// count is csr_pm_kernel's.  S is never a DMA target, and A's buffer is not
// re-issued before the barrier that opens the next stage (as there).
template <int T, int SF, int NBUF, int QPT, int OBJ = -1, int MODE = 0>
__global__ __launch_bounds__(T) void csr_pm_steps_kernel(const float* __restrict__ XT, int64_t ldx,
                                                         float* __restrict__ YT, int64_t ldy, int n_rows, int64_t P,
                                                         int xw, int sr, int qp_log2, int spt, int64_t n_stages,
                                                         int nseg, const int32_t* __restrict__ rowptr,
                                                         const int32_t* __restrict__ col,
                                                         const float* __restrict__ val, PmDgd e, int nw,
                                                         int mix_steps) {
  constexpr int kDma = SF / 4 / T;
  static_assert(kDma * 4 * T == SF, "a stage is a whole number of DMA rounds");
  extern __shared__ __attribute__((aligned(16))) float img[];  // NBUF x SF, then the scratch image (sr * xw)
  float* const scratch = img + NBUF * SF;
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int q0 = QPT == 1 ? (tid & ((1 << qp_log2) - 1)) : tid;
  const int g = QPT == 1 ? (tid >> qp_log2) : 0;
  const int GR = QPT == 1 ? (T >> qp_log2) : 1;
  const int nnz = rowptr[n_rows];
  Quad Q[QPT];
  if (nnz > 0) {
#pragma unroll
    for (int j = 0; j < QPT; ++j) load_quad(Q[j], q0 + j * T, n_rows, nnz, rowptr, col, val);
  } else {
#pragma unroll
    for (int j = 0; j < QPT; ++j) Q[j] = Quad{};
  }
  // stage order and ring as csr_pm_kernel
  const int64_t W = gridDim.x / nseg, seg = blockIdx.x % nseg, wl = blockIdx.x / nseg;
  const int64_t seg_len = (n_stages + nseg - 1) / nseg;
  const int64_t seg_n = std::max<int64_t>(0, std::min<int64_t>(seg_len, n_stages - seg * seg_len));
  const int64_t nk = wl < seg_n ? (seg_n - wl + W - 1) / W : 0;
  auto stage_of = [&](int64_t k) { return seg * seg_len + wl + k * W; };
  const int xq = xw / 4, xr4 = (n_rows + 3) / 4;
  const int nq4 = nw / 4, nr4 = (n_rows + 3) / 4;
  const int nX = sr * xq, nTM = sr * nq4;
  auto issue = [&](int64_t k) {
    issue_stage<T, SF, OBJ, MODE>(img + (k % NBUF) * SF, XT, ldx, P, stage_of(k) * sr, xq, xr4, nq4, nr4, nX, nTM, e,
                                  tid, wave);
  };
  constexpr int kStores = (OBJ >= 0 && MODE != 0) ? 2 : 1;
#pragma unroll
  for (int k = 0; k < NBUF - 1; ++k)
    if (k < nk) issue(k);
  for (int64_t k = 0; k < nk; ++k) {
    const int64_t ahead = std::min<int64_t>(nk - 1, k + NBUF - 2) - k;
    wait_vmcnt(static_cast<int>(std::min<int64_t>(63, kStores * spt * std::min<int64_t>(k, NBUF - 1) + kDma * ahead)));
    __builtin_amdgcn_s_barrier();  // stage k landed; buffer (k-1) % NBUF and the scratch image are free
    if (k + NBUF - 1 < nk) issue(k + NBUF - 1);
    const int64_t p0 = stage_of(k) * sr;
    float* const A = img + (k % NBUF) * SF;
    const int rows_here = static_cast<int>(std::min<int64_t>(sr, P - p0));
    float *cur = A, *nxt = scratch;
    for (int t = 1; t < mix_steps; ++t) {
      mix_image<T, QPT>(Q, cur, nxt, n_rows, rows_here, xw, spt, q0, g, GR, rowptr, col, val);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's reads of cur and writes of nxt are done
      __builtin_amdgcn_s_barrier();                       // ... and every wave's: nxt is whole, cur is free
      float* const was = cur;
      cur = nxt;
      nxt = was;
    }
    mix_stage<T, QPT, OBJ, MODE>(Q, cur, YT, ldy, n_rows, P, p0, xw, sr, spt, q0, g, GR, rowptr, col, val, e, nw,
                                 A + sr * xw);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// ----------------------------------------------------------------------------
// The gradient-tracking round (DIGing / NEXT) of config 3 in one pass:
//   x_i' = sum_j W_ij x_j - lr s_i
//   s_i' = sum_j W_ij s_j + grad f_i(x_i') - grad f_i(x_i)
// with W = W_off (CSR) + diag(self_w).  Not in the reference, which has no
// decentralised optimiser beyond the consensus round (DIST/simulators.py:
// 147-162); the mix is its consensus (DIST/clients.py:61-69).  Per coordinate:
//   ax = mix_quad over the X image, as = mix_quad over the S image (same Quad)
// and then gt_finish (dol_launch.h), the lane the agent-major rounds of
// gt_ring.hip and gt_csr.hip run too.  A stage holds sr p-rows of three
// images -- X and S xw floats each (both are gathered), T nw floats -- that
// come in by one LDS-DMA ring; the agent's own x, s, t are f4 LDS reads of the
// same images, so no gradient matrix is stored or streamed: X, S, T in, X', S'
// out, 5 x 4 bytes per coordinate.
// ----------------------------------------------------------------------------
struct PmGt {
  const float* S; int64_t ld_s;
  float* XO; int64_t ldxo;
  float* SO; int64_t ldso;
  const float* T; int64_t ldt;
  const float* D;  // self weights [n_rows] or NULL
  float neg_lr;
};

// four self weights of quad q from clamped addresses (as load_quad); zeros without D
__device__ __forceinline__ f4 load_self_weights(const float* __restrict__ D, int q, int n_rows) {
  if (!D) return f4{0.f, 0.f, 0.f, 0.f};
  float d[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) d[a] = D[min(4 * q + a, n_rows - 1)];
  return f4{d[0], d[1], d[2], d[3]};
}

// One stage of the round: the X images at im0, the S images behind them, the
// T images behind those; two buffer stores per (p-row, quad), dead lanes
// pointed out of range as in mix_stage.
template <int T, int OBJ>
__device__ __forceinline__ void gt_stage(const Quad (&Q)[1], f4 dw, const float* __restrict__ im0, const PmGt& e,
                                         int n_rows, int64_t P, int64_t p0, int xw, int nw, int sr, int spt, int q0,
                                         int g, int GR, const int32_t* __restrict__ rowptr,
                                         const int32_t* __restrict__ col, const float* __restrict__ val) {
  const int nq = (n_rows + 3) / 4;
  const int64_t rows_here = std::min<int64_t>(sr, P - p0);
  const rsrc_t rx = make_rsrc(e.XO + p0 * e.ldxo, static_cast<uint32_t>(rows_here * e.ldxo * 4));
  const rsrc_t rs = make_rsrc(e.SO + p0 * e.ldso, static_cast<uint32_t>(rows_here * e.ldso * 4));
  const float* sim0 = im0 + sr * xw;
  const float* tim0 = sim0 + sr * xw;
  const bool self = e.D != nullptr;
  const int q = q0;
  const int qc = q < nq ? q : 0;
  for (int u = 0; u < spt; ++u) {
    const int pr = g + u * GR;
    const bool prow_ok = pr < rows_here;
    const int prc = pr < sr ? pr : 0;
    const float* xim = im0 + prc * xw;
    const float* sim = sim0 + prc * xw;
    const f4 ax = mix_quad(Q[0], xim, q, rowptr, col, val);
    const f4 as = mix_quad(Q[0], sim, q, rowptr, col, val);
    const f4 xv = *reinterpret_cast<const f4*>(xim + 4 * qc);
    const f4 sv = *reinterpret_cast<const f4*>(sim + 4 * qc);
    const f4 tv = *reinterpret_cast<const f4*>(tim0 + prc * nw + 4 * qc);
    f4 xo, so;
    gt_finish<OBJ>(ax, as, xv, sv, tv, dw, self, e.neg_lr, xo, so);
    const uint32_t offx = static_cast<uint32_t>((pr * e.ldxo + 4 * q) * 4);
    const uint32_t offs = static_cast<uint32_t>((pr * e.ldso + 4 * q) * 4);
    if (4 * q + 3 < n_rows || q >= nq) {  // whole quad, or none (dropped)
      const bool ok = prow_ok && q < nq;
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4, xo), rx, ok ? offx : kOOB, 0, kNT);
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4, so), rs, ok ? offs : kOOB, 0, kNT);
    } else {  // the ragged last quad (elements named one by one: hipcc 7.2 stored
              // element 0 four times from a loop over y[a] here)
      const int left = n_rows - 4 * q;  // 1..3
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(xo.x), rx, prow_ok ? offx : kOOB, 0, kNT);
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(xo.y), rx, prow_ok && left > 1 ? offx + 4 : kOOB, 0,
                                            kNT);
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(xo.z), rx, prow_ok && left > 2 ? offx + 8 : kOOB, 0,
                                            kNT);
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(so.x), rs, prow_ok ? offs : kOOB, 0, kNT);
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(so.y), rs, prow_ok && left > 1 ? offs + 4 : kOOB, 0,
                                            kNT);
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(so.z), rs, prow_ok && left > 2 ? offs + 8 : kOOB, 0,
                                            kNT);
    }
  }
}

// T threads per workgroup, SF floats per stage buffer, NBUF buffers; one quad
// per thread (at most 4 T agents).  The ring, the counted wait and the stage
// order are csr_pm_kernel's; kStores = 2.
template <int T, int SF, int NBUF, int OBJ>
__global__ __launch_bounds__(T) void csr_pm_gt_kernel(const float* __restrict__ XT, int64_t ldx, int n_rows,
                                                      int64_t P, int xw, int sr, int qp_log2, int spt,
                                                      int64_t n_stages, int nseg,
                                                      const int32_t* __restrict__ rowptr,
                                                      const int32_t* __restrict__ col,
                                                      const float* __restrict__ val, PmGt e, int nw) {
  constexpr int kDma = SF / 4 / T;
  static_assert(kDma * 4 * T == SF, "a stage is a whole number of DMA rounds");
  extern __shared__ __attribute__((aligned(16))) float img[];  // NBUF x SF
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int q0 = tid & ((1 << qp_log2) - 1);
  const int g = tid >> qp_log2;
  const int GR = T >> qp_log2;
  const int nnz = rowptr[n_rows];
  Quad Q[1];
  if (nnz > 0) load_quad(Q[0], q0, n_rows, nnz, rowptr, col, val);
  else Q[0] = Quad{};
  const f4 dw = load_self_weights(e.D, q0, n_rows);

  const int64_t W = gridDim.x / nseg, seg = blockIdx.x % nseg, wl = blockIdx.x / nseg;
  const int64_t seg_len = (n_stages + nseg - 1) / nseg;
  const int64_t seg_n = std::max<int64_t>(0, std::min<int64_t>(seg_len, n_stages - seg * seg_len));
  const int64_t nk = wl < seg_n ? (seg_n - wl + W - 1) / W : 0;
  auto stage_of = [&](int64_t k) { return seg * seg_len + wl + k * W; };
  // This thread's kDma pieces of a stage, classified once: piece d is 16 B of
  // operand sel (0 X, 1 S, 2 T; 3 dead) in p-row pr of the stage, poff floats
  // from that operand's row p0 (pmeta = pr | sel << 16).  issue_stage keeps
  // about 11 registers per piece live across the stage loop; with three
  // operands and five pieces the kernel then spilled, hence the packing.
  const int xq = xw / 4, nq4 = nw / 4, nr4 = (n_rows + 3) / 4;
  const int nX = sr * xq, nTM = sr * nq4;
  int poff[kDma], pmeta[kDma];
#pragma unroll
  for (int d = 0; d < kDma; ++d) {
    const int pc = d * T + tid;
    int sel = 3, pr = 0, off = 0;
    if (pc < 2 * nX) {
      const int h = pc >= nX ? 1 : 0, ps = pc - h * nX;
      pr = ps / xq;
      const int j4 = ps - pr * xq;
      if (j4 < nr4) {
        sel = h;
        off = static_cast<int>(pr * (h ? e.ld_s : ldx)) + 4 * j4;
      }
    } else if (pc - 2 * nX < nTM) {
      const int pt = pc - 2 * nX;
      pr = pt / nq4;
      sel = 2;
      off = static_cast<int>(pr * e.ldt) + 4 * (pt - pr * nq4);
    }
    poff[d] = off;
    pmeta[d] = pr | sel << 16;
  }
  auto issue = [&](int64_t k) {  // stage k of this workgroup -> buffer k % NBUF; dead pieces re-read XT[0..3]
    float* dst = img + (k % NBUF) * SF;
    const int64_t p0 = stage_of(k) * sr;
    const float* bx = XT + p0 * ldx;
    const float* bs = e.S + p0 * e.ld_s;
    const float* bt = e.T + p0 * e.ldt;
#pragma unroll
    for (int d = 0; d < kDma; ++d) {
      const int sel = pmeta[d] >> 16, pr = pmeta[d] & 0xffff;
      const float* base = sel == 0 ? bx : sel == 1 ? bs : bt;
      const float* src = sel != 3 && p0 + pr < P ? base + poff[d] : XT;
      __builtin_amdgcn_global_load_lds(DOL_GPTR(src), DOL_LPTR(dst + (d * T + wave * 64) * 4), 16, 0, kNT);
    }
  };
  constexpr int kStores = 2;  // buffer stores per (p-row, quad): X' and S'
#pragma unroll
  for (int k = 0; k < NBUF - 1; ++k)
    if (k < nk) issue(k);
  for (int64_t k = 0; k < nk; ++k) {
    const int64_t ahead = std::min<int64_t>(nk - 1, k + NBUF - 2) - k;
    wait_vmcnt(static_cast<int>(std::min<int64_t>(63, kStores * spt * std::min<int64_t>(k, NBUF - 1) + kDma * ahead)));
    __builtin_amdgcn_s_barrier();  // every wave's share landed; buffer (k-1) % NBUF is free
    if (k + NBUF - 1 < nk) issue(k + NBUF - 1);
    gt_stage<T, OBJ>(Q, dw, img + (k % NBUF) * SF, e, n_rows, P, stage_of(k) * sr, xw, nw, sr, spt, q0, g, GR, rowptr,
                     col, val);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this stage's LDS reads are done before the next barrier
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// ----------------------------------------------------------------------------
// The EXTRA round of config 3 in one pass (extra_finish, dol_launch.h):
//   x_i' = sum_j W_ij x_j - lr grad f_i(x_i) - c_i
//   c_i' = c_i + (x_i - sum_j W_ij x_j) / 2
// with W = W_off (CSR) + diag(self_w).  Not in the reference (as the
// gradient-tracking round above); the mix is its consensus
// (DIST/clients.py:61-69).  Only X is gathered: a stage is the DGD round's
// mode-2 stage with the correction where the momentum is -- sr p-rows of X
// images (xw floats each), then of T images, then of C images (nw floats each)
// -- brought in by one LDS-DMA ring.  The centre x is an f4 LDS read of the X
// image, t and c of theirs.  X' goes to YT and c' back to C in place: a C
// p-row is read (by DMA) and written by the one workgroup that owns its stage,
// and the write is issued after the barrier that retires the stage's DMA, as
// the momentum's is in csr_pm_kernel.  X, T, C in, X', C' out: 5 x 4 bytes per
// coordinate.
// ----------------------------------------------------------------------------
struct PmExtra {
  float* YT; int64_t ldy;
  const float* T; int64_t ldt;
  float* C; int64_t ldc;
  const float* D;  // self weights [n_rows] or NULL
  float neg_lr;
};

// One stage of the round: the X images at im0, the T images behind them, the
// C images behind those; two buffer stores per (p-row, quad), dead lanes
// pointed out of range as in mix_stage.
template <int T, int OBJ>
__device__ __forceinline__ void extra_stage(const Quad (&Q)[1], f4 dw, const float* __restrict__ im0, const PmExtra& e,
                                            int n_rows, int64_t P, int64_t p0, int xw, int nw, int sr, int spt, int q0,
                                            int g, int GR, const int32_t* __restrict__ rowptr,
                                            const int32_t* __restrict__ col, const float* __restrict__ val) {
  const int nq = (n_rows + 3) / 4;
  const int64_t rows_here = std::min<int64_t>(sr, P - p0);
  const rsrc_t ry = make_rsrc(e.YT + p0 * e.ldy, static_cast<uint32_t>(rows_here * e.ldy * 4));
  const rsrc_t rc = make_rsrc(e.C + p0 * e.ldc, static_cast<uint32_t>(rows_here * e.ldc * 4));
  const float* tim0 = im0 + sr * xw;
  const float* cim0 = tim0 + sr * nw;
  const bool self = e.D != nullptr;
  const int q = q0;
  const int qc = q < nq ? q : 0;
  for (int u = 0; u < spt; ++u) {
    const int pr = g + u * GR;
    const bool prow_ok = pr < rows_here;
    const int prc = pr < sr ? pr : 0;
    const float* xim = im0 + prc * xw;
    const f4 ax = mix_quad(Q[0], xim, q, rowptr, col, val);
    const f4 xv = *reinterpret_cast<const f4*>(xim + 4 * qc);
    const f4 tv = *reinterpret_cast<const f4*>(tim0 + prc * nw + 4 * qc);
    const f4 cv = *reinterpret_cast<const f4*>(cim0 + prc * nw + 4 * qc);
    f4 xo, co;
    extra_finish<OBJ>(ax, xv, cv, tv, dw, self, e.neg_lr, xo, co);
    const uint32_t offy = static_cast<uint32_t>((pr * e.ldy + 4 * q) * 4);
    const uint32_t offc = static_cast<uint32_t>((pr * e.ldc + 4 * q) * 4);
    if (4 * q + 3 < n_rows || q >= nq) {  // whole quad, or none (dropped)
      const bool ok = prow_ok && q < nq;
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4, xo), ry, ok ? offy : kOOB, 0, kNT);
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4, co), rc, ok ? offc : kOOB, 0, kNT);
    } else {  // the ragged last quad (elements named one by one: hipcc 7.2 stored
              // element 0 four times from a loop over y[a] here)
      const int left = n_rows - 4 * q;  // 1..3
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(xo.x), ry, prow_ok ? offy : kOOB, 0, kNT);
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(xo.y), ry, prow_ok && left > 1 ? offy + 4 : kOOB, 0,
                                            kNT);
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(xo.z), ry, prow_ok && left > 2 ? offy + 8 : kOOB, 0,
                                            kNT);
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(co.x), rc, prow_ok ? offc : kOOB, 0, kNT);
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(co.y), rc, prow_ok && left > 1 ? offc + 4 : kOOB, 0,
                                            kNT);
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(co.z), rc, prow_ok && left > 2 ? offc + 8 : kOOB, 0,
                                            kNT);
    }
  }
}

// T threads per workgroup, SF floats per stage buffer, NBUF buffers; one quad
// per thread (at most 4 T agents).  The ring, the counted wait, the stage order
// and the packed stage issue are csr_pm_gt_kernel's; kStores = 2.
template <int T, int SF, int NBUF, int OBJ>
__global__ __launch_bounds__(T) void csr_pm_extra_kernel(const float* __restrict__ XT, int64_t ldx, int n_rows,
                                                         int64_t P, int xw, int sr, int qp_log2, int spt,
                                                         int64_t n_stages, int nseg,
                                                         const int32_t* __restrict__ rowptr,
                                                         const int32_t* __restrict__ col,
                                                         const float* __restrict__ val, PmExtra e, int nw) {
  constexpr int kDma = SF / 4 / T;
  static_assert(kDma * 4 * T == SF, "a stage is a whole number of DMA rounds");
  extern __shared__ __attribute__((aligned(16))) float img[];  // NBUF x SF
  const int tid = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int q0 = tid & ((1 << qp_log2) - 1);
  const int g = tid >> qp_log2;
  const int GR = T >> qp_log2;
  const int nnz = rowptr[n_rows];
  Quad Q[1];
  if (nnz > 0) load_quad(Q[0], q0, n_rows, nnz, rowptr, col, val);
  else Q[0] = Quad{};
  const f4 dw = load_self_weights(e.D, q0, n_rows);

  const int64_t W = gridDim.x / nseg, seg = blockIdx.x % nseg, wl = blockIdx.x / nseg;
  const int64_t seg_len = (n_stages + nseg - 1) / nseg;
  const int64_t seg_n = std::max<int64_t>(0, std::min<int64_t>(seg_len, n_stages - seg * seg_len));
  const int64_t nk = wl < seg_n ? (seg_n - wl + W - 1) / W : 0;
  auto stage_of = [&](int64_t k) { return seg * seg_len + wl + k * W; };
  // This thread's kDma pieces of a stage, classified once as in
  // csr_pm_gt_kernel: piece d is 16 B of operand sel (0 X, 1 T, 2 C; 3 dead) in
  // p-row pr of the stage, poff floats from that operand's row p0.
  const int xq = xw / 4, nq4 = nw / 4, nr4 = (n_rows + 3) / 4;
  const int nX = sr * xq, nTM = sr * nq4;
  int poff[kDma], pmeta[kDma];
#pragma unroll
  for (int d = 0; d < kDma; ++d) {
    const int pc = d * T + tid;
    int sel = 3, pr = 0, off = 0;
    if (pc < nX) {
      pr = pc / xq;
      const int j4 = pc - pr * xq;
      if (j4 < nr4) {
        sel = 0;
        off = static_cast<int>(pr * ldx) + 4 * j4;
      }
    } else if (pc - nX < 2 * nTM) {
      const int pt = pc - nX, h = pt >= nTM ? 1 : 0, r = pt - h * nTM;
      pr = r / nq4;
      sel = 1 + h;
      off = static_cast<int>(pr * (h ? e.ldc : e.ldt)) + 4 * (r - pr * nq4);
    }
    poff[d] = off;
    pmeta[d] = pr | sel << 16;
  }
  auto issue = [&](int64_t k) {  // stage k of this workgroup -> buffer k % NBUF; dead pieces re-read XT[0..3]
    float* dst = img + (k % NBUF) * SF;
    const int64_t p0 = stage_of(k) * sr;
    const float* bx = XT + p0 * ldx;
    const float* bt = e.T + p0 * e.ldt;
    const float* bc = e.C + p0 * e.ldc;
#pragma unroll
    for (int d = 0; d < kDma; ++d) {
      const int sel = pmeta[d] >> 16, pr = pmeta[d] & 0xffff;
      const float* base = sel == 0 ? bx : sel == 1 ? bt : bc;
      const float* src = sel != 3 && p0 + pr < P ? base + poff[d] : XT;
      __builtin_amdgcn_global_load_lds(DOL_GPTR(src), DOL_LPTR(dst + (d * T + wave * 64) * 4), 16, 0, kNT);
    }
  };
  constexpr int kStores = 2;  // buffer stores per (p-row, quad): X' and C'
#pragma unroll
  for (int k = 0; k < NBUF - 1; ++k)
    if (k < nk) issue(k);
  for (int64_t k = 0; k < nk; ++k) {
    const int64_t ahead = std::min<int64_t>(nk - 1, k + NBUF - 2) - k;
    wait_vmcnt(static_cast<int>(std::min<int64_t>(63, kStores * spt * std::min<int64_t>(k, NBUF - 1) + kDma * ahead)));
    __builtin_amdgcn_s_barrier();  // every wave's share landed (the C images too: their p-rows may be written now);
                                   // buffer (k-1) % NBUF is free
    if (k + NBUF - 1 < nk) issue(k + NBUF - 1);
    extra_stage<T, OBJ>(Q, dw, img + (k % NBUF) * SF, e, n_rows, P, stage_of(k) * sr, xw, nw, sr, spt, q0, g, GR,
                        rowptr, col, val);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this stage's LDS reads are done before the next barrier
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// G = g(X, T) elementwise over rows x cols (V = f4 columns or the scalar tail
// from c_off), row loads and stores nontemporal; either bank layout.
template <typename V, int OBJ>
__global__ __launch_bounds__(256) void separable_grad_kernel(const float* X, int64_t ldx, const float* Tg, int64_t ldt,
                                                             float* G, int64_t ldg, int64_t c_off,
                                                             int64_t ncols_v, int64_t n_col_tiles) {
  const int64_t blk = blockIdx.x;
  const int64_t r = blk / n_col_tiles;
  const int64_t c = (blk % n_col_tiles) * 256 + threadIdx.x;
  if (c >= ncols_v) return;
  const V x = ldv<V, true>(reinterpret_cast<const V*>(X + r * ldx + c_off) + c);
  const V t = ldv<V, true>(reinterpret_cast<const V*>(Tg + r * ldt + c_off) + c);
  V gv;
  if constexpr (Vec<V>::W == 1) {
    gv = separable_grad<OBJ>(x, t);
  } else {
    gv = V{separable_grad<OBJ>(x.x, t.x), separable_grad<OBJ>(x.y, t.y), separable_grad<OBJ>(x.z, t.z),
           separable_grad<OBJ>(x.w, t.w)};
  }
  stv<V, true>(reinterpret_cast<V*>(G + r * ldg + c_off) + c, gv);
}

// ----------------------------------------------------------------------------
// Tiled transpose B[c][r] = A[r][c] (fp32, 64 x 64 tiles through LDS, rows
// padded by one float against bank conflicts): converts the agent-major bank
// to the parameter-major one and back (setup / checkpoint time, not per round).
// ----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void transpose_kernel(const float* __restrict__ A, int64_t lda,
                                                        float* __restrict__ B, int64_t ldb, int64_t rows,
                                                        int64_t cols, int64_t tiles_c) {
  __shared__ float t[64][65];
  const int64_t tr = blockIdx.x / tiles_c, tc = blockIdx.x % tiles_c;
  const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
  const int64_t r0 = tr * 64, c0 = tc * 64;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int64_t r = r0 + ly + 4 * i, c = c0 + lx;
    if (r < rows && c < cols) t[ly + 4 * i][lx] = A[r * lda + c];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int64_t c = c0 + ly + 4 * i, r = r0 + lx;
    if (r < rows && c < cols) B[c * ldb + r] = t[lx][ly + 4 * i];
  }
}

// stage order set by dol_pm_set_stage_order (0: DOL_PM_NSEG, else 8); atomic,
// and the _ex entry points take the order per call
std::atomic<int> g_pm_nseg{0};

}  // namespace

extern "C" {

// The best stage order depends on where the bank's pages landed: on one box,
// process to process, the same mix took 13.35 ms at 8 segments and 12.94 at 32
// in one process and 11.79 / 12.31 in the next (tools/pm_nseg_sweep.py,
// profiles/r03_pm_stage_order.txt); dolhip.ops.tune_pm_stage_order picks it per
// process for the buffers at hand.
int dol_pm_set_stage_order(int32_t nseg) {
  if (nseg < 0 || nseg > 256) return fail(DOL_EINVAL, "dol_pm_set_stage_order: segments %d outside [0, 256]", nseg);
  const int prev = g_pm_nseg.exchange(nseg, std::memory_order_relaxed);
  dol::g_err[0] = '\0';
  return prev;
}

}  // extern "C"

namespace {

// obj < 0: the plain mix; else the config-3 round (epilogue e, momentum mode).
// mix_steps > 1: W^mix_steps in one pass (csr_pm_steps_kernel; W square, the
// callers pass x_rows == n_rows); 1 is the single-step kernel, launched as ever.
int mix_csr_pm_impl(const char* nm, const float* XT, int64_t ldx, int32_t x_rows, float* YT, int64_t ldy,
                    int32_t n_rows, int64_t P, const int32_t* rowptr, const int32_t* col, const float* val, int obj,
                    int mode, const PmDgd& e, int32_t nseg_req, hipStream_t s, int mix_steps = 1) {
  if (mix_steps < 1 || mix_steps > DOL_PM_MAX_FUSED_STEPS)
    return fail(DOL_EINVAL, "%s: %d mixing steps outside [1, %d] (the cap bounds one launch's run time)", nm,
                mix_steps, DOL_PM_MAX_FUSED_STEPS);
  if (nseg_req < 0 || nseg_req > 256) return fail(DOL_EINVAL, "%s: stage order %d outside [0, 256]", nm, nseg_req);
  if (n_rows < 0 || x_rows < 0 || P < 0) return fail(DOL_EINVAL, "%s: negative size", nm);
  if (n_rows == 0 || P == 0) { dol::g_err[0] = '\0'; return DOL_OK; }
  if (!XT || !YT || !rowptr || (x_rows > 0 && (!col || !val))) return fail(DOL_EINVAL, "%s: null pointer", nm);
  if (x_rows < 1) return fail(DOL_EINVAL, "%s: x_rows must be >= 1", nm);
  if (x_rows > kMaxAgents || n_rows > kMaxAgents)
    return fail(DOL_EINVAL, "%s: at most %d agents (x_rows %d, n_rows %d)", nm, kMaxAgents, x_rows, n_rows);
  if (ldx % 4 || ldx < (x_rows + 3) / 4 * 4 || ldy % 4 || ldy < (n_rows + 3) / 4 * 4)
    return fail(DOL_EINVAL, "%s: ldx / ldy must be multiples of 4 covering the rounded-up agent counts", nm);
  if ((reinterpret_cast<uintptr_t>(XT) | reinterpret_cast<uintptr_t>(YT)) & 15u)
    return fail(DOL_EINVAL, "%s: XT and YT must be 16-B aligned", nm);
  if (XT == YT) return fail(DOL_EINVAL, "%s: XT and YT alias (Jacobi mix needs two buffers)", nm);
  const int xw = (x_rows + 255) / 256 * 256;
  const int nq = (n_rows + 3) / 4;
  const int nw = 4 * nq;                                  // epilogue image width (floats)
  const int ne = obj < 0 ? 0 : (mode == 2 ? 2 : 1);       // epilogue operands staged per p-row
  if (obj >= 0) {
    if (!e.T || (mode != 0 && !e.M)) return fail(DOL_EINVAL, "%s: null target / momentum", nm);
    if (e.ldt % 4 || e.ldt < nw || (mode != 0 && (e.ldm % 4 || e.ldm < nw)))
      return fail(DOL_EINVAL, "%s: ldt / ldm must be multiples of 4 covering the rounded-up agent count", nm);
    if ((reinterpret_cast<uintptr_t>(e.T) | (mode ? reinterpret_cast<uintptr_t>(e.M) : 0)) & 15u)
      return fail(DOL_EINVAL, "%s: target / momentum must be 16-B aligned", nm);
    if (nq > kT1 || xw > 4096) return fail(DOL_EINVAL, "%s: the fused round takes at most 4096 agents", nm);
  }
  // geometry: 1024-thread workgroups, one per CU.  Up to 4096 agents (one quad
  // per thread): 64 KiB stages, 2 buffers; beyond (two quads per thread, a
  // p-row up to 32 KiB): 32 KiB stages, 5 buffers (r02; 4 in r01).  Measured at 1024 x 2^20
  // (one box): 64 KiB x 2 1.511 ms, 32 KiB x 4 1.533, 48 KiB x 3 1.541;
  // 256- / 512-thread workgroups (8 / 16 KiB stages, 2-4 per CU) 1.82 / 1.64;
  // one stage per short-lived workgroup 4.4; a per-wave ring (no workgroup
  // barrier, 4 KiB p-rows, 176 VGPRs) 1.64.
  const bool big = nq > kT1 || xw > 4096;
  const bool multi = mix_steps > 1;
  // fused round (<= 4096 agents): 64 KiB x 2 stages, or 80 KiB x 2 with the
  // momentum read (mode 2).  Beyond 4096 agents: five 32-KiB buffers (all 160
  // KiB, four p-rows in flight; profiles/r02_pm_nbuf.txt).  At <= 4096 agents
  // 5 x 32 KiB ran level with 2 x 64 KiB (1.56-1.59 ms at 1024 x 2^20).
  // Multi-step (csr_pm_steps_kernel): the ring plus one scratch image of the
  // stage's X part.  Up to 4096 agents 48 KiB x 2 + <= 48 KiB for the mix and
  // every mode of the round (at 4096 agents with momentum: X, target and
  // momentum p-row = one 48 KiB stage, 16 KiB scratch); beyond, 32 KiB x 4 +
  // 32 KiB, the whole 160 KiB.
  const int SF = multi ? (big ? 8192 : 12288) : big ? 8192 : (ne == 2 ? 20480 : 16384);
  const int NB = multi ? (big ? 4 : 2) : big ? 5 : 2;  // must match the kernel's NBUF (LDS size)
  int sr = SF / (xw + ne * nw);
  int qp_log2 = 0, spt;
  if (!big) {
    while ((1 << qp_log2) < nq) ++qp_log2;
    const int gr = kT1 >> qp_log2;
    if (sr >= gr) sr = std::min(sr / gr * gr, 4 * gr);
    spt = (sr + gr - 1) / gr;
  } else {
    sr = 1;
    spt = 2;
  }
  if (sr < 1) return fail(DOL_EINVAL, "%s: a p-row and its epilogue operands exceed a stage", nm);
  if (int64_t(sr) * std::max(ldy, std::max(e.ldt, e.ldm)) * 4 >= (int64_t(1) << 31))
    return fail(DOL_EINVAL, "%s: leading dimension too large", nm);
  const int64_t n_stages = (P + sr - 1) / sr;
  const int ncu = n_cus();
  if (ncu <= 0) return fail(DOL_EINVAL, "%s: no device", nm);
  const int64_t grid = std::min<int64_t>(ncu, n_stages);
  const int proc = g_pm_nseg.load(std::memory_order_relaxed);
  int nseg = nseg_req > 0 ? nseg_req : proc > 0 ? proc : env_int("DOL_PM_NSEG", 8);
  if (nseg < 1 || grid % nseg) nseg = 1;
  auto go_steps = [&](auto kern) {
    const int lds = (NB * SF + sr * xw) * 4;  // the ring, then the scratch image
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(grid)), dim3(kT1), lds, s, XT, ldx, YT, ldy, n_rows, P, xw, sr,
                       qp_log2, spt, n_stages, nseg, rowptr, col, val, e, nw, mix_steps);
  };
  if (multi) {
    if (obj < 0) {
      if (big) go_steps(csr_pm_steps_kernel<kT1, 8192, 4, 2>);
      else go_steps(csr_pm_steps_kernel<kT1, 12288, 2, 1>);
    } else {
      dispatch([&](auto oc, auto mc) {
        go_steps(csr_pm_steps_kernel<kT1, 12288, 2, 1, decltype(oc)::value, decltype(mc)::value>);
      }, Ints<0, 1>{obj}, Ints<0, 1, 2>{mode});
    }
    return check_launch(nm);
  }
  auto go = [&](auto kern) {
    const int lds = NB * SF * 4;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    static const int wait_mode = env_int("DOL_PM_WAIT", 1);
    hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(grid)), dim3(kT1), lds, s, XT, ldx, x_rows, YT, ldy, n_rows, P,
                       xw, sr, qp_log2, spt, n_stages, nseg, rowptr, col, val, e, nw, wait_mode);
  };
  if (obj < 0) {
    if (big) go(csr_pm_kernel<kT1, 8192, 5, 2>);
    else go(csr_pm_kernel<kT1, 16384, 2, 1>);
  } else {  // small geometry only; mode 2 stages the momentum image too
    dispatch([&](auto oc, auto mc) {
      constexpr int O = decltype(oc)::value, M = decltype(mc)::value;
      go(csr_pm_kernel<kT1, (M == 2 ? 20480 : 16384), 2, 1, O, M>);
    }, Ints<0, 1>{obj}, Ints<0, 1, 2>{mode});
  }
  return check_launch(nm);
}

constexpr int kGtMaxAgents = 4 * kT1;  // one quad per thread

// The gradient-tracking round: validation in mix_csr_pm_impl's order, then
// csr_pm_gt_kernel in the small geometry (1024-thread workgroups, one per CU,
// one quad per thread).  It keeps its own validation rather than GtRows
// (dol_launch.h): the objective comes first here, the leading dimensions cover
// agents not P, alignment is required, and the messages name XT, ST and TT.
int gt_csr_pm_impl(const char* nm, const float* XT, int64_t ldx, const float* ST, int64_t ld_s, float* XO,
                   int64_t ldxo, float* SO, int64_t ldso, int32_t n, int64_t P, const int32_t* rowptr,
                   const int32_t* col, const float* val, const float* self_w, const float* TT, int64_t ldt,
                   int32_t objective, float lr, int32_t nseg_req, hipStream_t s) {
  if (objective != 0 && objective != 1) return fail(DOL_EINVAL, "%s: objective must be 0 or 1", nm);
  if (nseg_req < 0 || nseg_req > 256) return fail(DOL_EINVAL, "%s: stage order %d outside [0, 256]", nm, nseg_req);
  if (n < 0 || P < 0) return fail(DOL_EINVAL, "%s: negative size", nm);
  if (n == 0 || P == 0) { dol::g_err[0] = '\0'; return DOL_OK; }
  if (!XT || !ST || !XO || !SO || !TT || !rowptr || !col || !val) return fail(DOL_EINVAL, "%s: null pointer", nm);
  if (n > kGtMaxAgents)
    return fail(DOL_EINVAL, "%s: the gradient-tracking round takes at most %d agents (got %d)", nm, kGtMaxAgents, n);
  const int nq = (n + 3) / 4;
  const int nw = 4 * nq;
  for (const int64_t ld : {ldx, ld_s, ldxo, ldso, ldt})
    if (ld % 4 || ld < nw)
      return fail(DOL_EINVAL, "%s: leading dimensions must be multiples of 4 covering the rounded-up agent count", nm);
  if ((reinterpret_cast<uintptr_t>(XT) | reinterpret_cast<uintptr_t>(ST) | reinterpret_cast<uintptr_t>(XO) |
       reinterpret_cast<uintptr_t>(SO) | reinterpret_cast<uintptr_t>(TT)) & 15u)
    return fail(DOL_EINVAL, "%s: XT, ST, XO, SO and TT must be 16-B aligned", nm);
  if (XT == ST || XT == XO || XT == SO || ST == XO || ST == SO || XO == SO)
    return fail(DOL_EINVAL, "%s: XT, ST, XO and SO alias (a Jacobi update of both needs four buffers)", nm);
  // geometry: X + S + T p-rows per stage, 2 xw + nw floats each (48 KiB at
  // 4096 agents, so every agent count fits either ring): 80 KiB x 2 for least
  // squares, 48 KiB x 3 for logistic, the rings that won (the file's header)
  const int xw = (n + 255) / 256 * 256;
  const int SF = objective == 0 ? 20480 : 12288;
  const int NB = objective == 0 ? 2 : 3;  // must match the kernel's NBUF (LDS size)
  int sr = SF / (2 * xw + nw);
  int qp_log2 = 0;
  while ((1 << qp_log2) < nq) ++qp_log2;
  const int gr = kT1 >> qp_log2;
  if (sr >= gr) sr = std::min(sr / gr * gr, 4 * gr);
  const int spt = (sr + gr - 1) / gr;
  if (sr < 1) return fail(DOL_EINVAL, "%s: a p-row of X, S and T exceeds a stage", nm);
  // a stage's offsets are 32-bit: the stores' buffer offsets and the DMA pieces' float offsets
  if (int64_t(sr) * std::max({ldx, ld_s, ldxo, ldso, ldt}) * 4 >= (int64_t(1) << 31))
    return fail(DOL_EINVAL, "%s: leading dimension too large", nm);
  const int64_t n_stages = (P + sr - 1) / sr;
  const int ncu = n_cus();
  if (ncu <= 0) return fail(DOL_EINVAL, "%s: no device", nm);
  const int64_t grid = std::min<int64_t>(ncu, n_stages);
  const int proc = g_pm_nseg.load(std::memory_order_relaxed);
  int nseg = nseg_req > 0 ? nseg_req : proc > 0 ? proc : env_int("DOL_PM_NSEG", 8);
  if (nseg < 1 || grid % nseg) nseg = 1;
  const PmGt e{ST, ld_s, XO, ldxo, SO, ldso, TT, ldt, self_w, -lr};
  auto go = [&](auto kern) {
    const int lds = NB * SF * 4;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(grid)), dim3(kT1), lds, s, XT, ldx, n, P, xw, sr, qp_log2, spt,
                       n_stages, nseg, rowptr, col, val, e, nw);
  };
  if (objective == 0) go(csr_pm_gt_kernel<kT1, 20480, 2, 0>);
  else go(csr_pm_gt_kernel<kT1, 12288, 3, 1>);
  return check_launch(nm);
}

// The EXTRA round: validation in gt_csr_pm_impl's order and wording, then
// csr_pm_extra_kernel in the small geometry (1024-thread workgroups, one per
// CU, one quad per thread).
int extra_csr_pm_impl(const char* nm, const float* XT, int64_t ldx, float* YT, int64_t ldy, int32_t n, int64_t P,
                      const int32_t* rowptr, const int32_t* col, const float* val, const float* self_w,
                      const float* TT, int64_t ldt, float* CT, int64_t ldc, int32_t objective, float lr,
                      int32_t nseg_req, hipStream_t s) {
  if (objective != 0 && objective != 1) return fail(DOL_EINVAL, "%s: objective must be 0 or 1", nm);
  if (nseg_req < 0 || nseg_req > 256) return fail(DOL_EINVAL, "%s: stage order %d outside [0, 256]", nm, nseg_req);
  if (n < 0 || P < 0) return fail(DOL_EINVAL, "%s: negative size", nm);
  if (n == 0 || P == 0) { dol::g_err[0] = '\0'; return DOL_OK; }
  if (!XT || !YT || !TT || !CT || !rowptr || !col || !val) return fail(DOL_EINVAL, "%s: null pointer", nm);
  if (n > kGtMaxAgents)
    return fail(DOL_EINVAL, "%s: the EXTRA round takes at most %d agents (got %d)", nm, kGtMaxAgents, n);
  const int nq = (n + 3) / 4;
  const int nw = 4 * nq;
  for (const int64_t ld : {ldx, ldy, ldt, ldc})
    if (ld % 4 || ld < nw)
      return fail(DOL_EINVAL, "%s: leading dimensions must be multiples of 4 covering the rounded-up agent count", nm);
  if ((reinterpret_cast<uintptr_t>(XT) | reinterpret_cast<uintptr_t>(YT) | reinterpret_cast<uintptr_t>(TT) |
       reinterpret_cast<uintptr_t>(CT)) & 15u)
    return fail(DOL_EINVAL, "%s: XT, YT, TT and CT must be 16-B aligned", nm);
  if (XT == YT) return fail(DOL_EINVAL, "%s: XT and YT alias (Jacobi mix needs two buffers)", nm);
  if (CT == XT || CT == YT || CT == TT)
    return fail(DOL_EINVAL, "%s: CT aliases XT, YT or TT (the correction is updated in place)", nm);
  // geometry: X + T + C p-rows per stage, xw + 2 nw floats each (48 KiB at
  // 4096 agents, so every agent count fits): 48 KiB x 3 for both objectives,
  // the ring that won at 1024 x 2^20 (the file's header)
  const int xw = (n + 255) / 256 * 256;
  constexpr int SF = 12288, NB = 3;  // the kernel's SF and NBUF (LDS size)
  int sr = SF / (xw + 2 * nw);
  int qp_log2 = 0;
  while ((1 << qp_log2) < nq) ++qp_log2;
  const int gr = kT1 >> qp_log2;
  if (sr >= gr) sr = std::min(sr / gr * gr, 4 * gr);
  const int spt = (sr + gr - 1) / gr;
  if (sr < 1) return fail(DOL_EINVAL, "%s: a p-row of X, T and C exceeds a stage", nm);
  // a stage's offsets are 32-bit: the stores' buffer offsets and the DMA pieces' float offsets
  if (int64_t(sr) * std::max({ldx, ldy, ldt, ldc}) * 4 >= (int64_t(1) << 31))
    return fail(DOL_EINVAL, "%s: leading dimension too large", nm);
  const int64_t n_stages = (P + sr - 1) / sr;
  const int ncu = n_cus();
  if (ncu <= 0) return fail(DOL_EINVAL, "%s: no device", nm);
  const int64_t grid = std::min<int64_t>(ncu, n_stages);
  const int proc = g_pm_nseg.load(std::memory_order_relaxed);
  int nseg = nseg_req > 0 ? nseg_req : proc > 0 ? proc : env_int("DOL_PM_NSEG", 8);
  if (nseg < 1 || grid % nseg) nseg = 1;
  const PmExtra e{YT, ldy, TT, ldt, CT, ldc, self_w, -lr};
  auto go = [&](auto kern) {
    const int lds = NB * SF * 4;
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    hipLaunchKernelGGL(kern, dim3(static_cast<unsigned>(grid)), dim3(kT1), lds, s, XT, ldx, n, P, xw, sr, qp_log2, spt,
                       n_stages, nseg, rowptr, col, val, e, nw);
  };
  dispatch([&](auto oc) { go(csr_pm_extra_kernel<kT1, SF, NB, decltype(oc)::value>); }, Ints<0, 1>{objective});
  return check_launch(nm);
}

}  // namespace

extern "C" {

int dol_gt_csr_pm_f32(const float* XT, int64_t ldx, const float* ST, int64_t lds, float* XO, int64_t ldxo, float* SO,
                      int64_t ldso, int32_t n, int64_t P, const int32_t* rowptr, const int32_t* col,
                      const float* val, const float* self_w, const float* TT, int64_t ldt, int32_t objective,
                      float lr, hipStream_t s) {
  return dol_gt_csr_pm_ex_f32(XT, ldx, ST, lds, XO, ldxo, SO, ldso, n, P, rowptr, col, val, self_w, TT, ldt, objective,
                              lr, 0, s);
}

int dol_gt_csr_pm_ex_f32(const float* XT, int64_t ldx, const float* ST, int64_t lds, float* XO, int64_t ldxo,
                         float* SO, int64_t ldso, int32_t n, int64_t P, const int32_t* rowptr, const int32_t* col,
                         const float* val, const float* self_w, const float* TT, int64_t ldt, int32_t objective,
                         float lr, int32_t nseg, hipStream_t s) {
  DOL_DIMS_OK("dol_gt_csr_pm_f32", ldx, lds, ldxo, ldso, ldt, P);
  return gt_csr_pm_impl("dol_gt_csr_pm_f32", XT, ldx, ST, lds, XO, ldxo, SO, ldso, n, P, rowptr, col, val, self_w, TT,
                        ldt, objective, lr, nseg, s);
}

int dol_extra_csr_pm_f32(const float* XT, int64_t ldx, float* YT, int64_t ldy, int32_t n, int64_t P,
                         const int32_t* rowptr, const int32_t* col, const float* val, const float* self_w,
                         const float* TT, int64_t ldt, float* CT, int64_t ldc, int32_t objective, float lr,
                         hipStream_t s) {
  return dol_extra_csr_pm_ex_f32(XT, ldx, YT, ldy, n, P, rowptr, col, val, self_w, TT, ldt, CT, ldc, objective, lr, 0,
                                 s);
}

int dol_extra_csr_pm_ex_f32(const float* XT, int64_t ldx, float* YT, int64_t ldy, int32_t n, int64_t P,
                            const int32_t* rowptr, const int32_t* col, const float* val, const float* self_w,
                            const float* TT, int64_t ldt, float* CT, int64_t ldc, int32_t objective, float lr,
                            int32_t nseg, hipStream_t s) {
  DOL_DIMS_OK("dol_extra_csr_pm_f32", ldx, ldy, ldt, ldc, P);
  return extra_csr_pm_impl("dol_extra_csr_pm_f32", XT, ldx, YT, ldy, n, P, rowptr, col, val, self_w, TT, ldt, CT, ldc,
                           objective, lr, nseg, s);
}

int dol_separable_grad_f32(const float* X, int64_t ldx, const float* T, int64_t ldt, float* G, int64_t ldg,
                           int64_t rows, int64_t cols, int32_t objective, hipStream_t s) {
  const char* nm = "dol_separable_grad_f32";
  DOL_DIMS_OK(nm, ldx, ldt, ldg, rows, cols);
  if (objective != 0 && objective != 1) return fail(DOL_EINVAL, "%s: objective must be 0 or 1", nm);
  DOL_CHECKED(check_rows(nm, rows < 0 || cols < 0, rows == 0 || cols == 0, !X || !T || !G,
                         ldx < cols || ldt < cols || ldg < cols, false, "", "ld < cols"));
  const ColSplit cs = split_cols(cols, row_vec_ok(X, ldx) && row_vec_ok(T, ldt) && row_vec_ok(G, ldg));
  if (mul_sat(cdiv(cs.n4 + cs.tail, 256), rows) > kMaxBlocks) return fail(DOL_EINVAL, "%s: too large", nm);
  auto launch = [&](auto vtag, int64_t c_off, int64_t nc) {
    using V = decltype(vtag);
    const int64_t nct = cdiv(nc, 256);
    dispatch([&](auto oc) {
      hipLaunchKernelGGL((separable_grad_kernel<V, decltype(oc)::value>), dim3(static_cast<unsigned>(nct * rows)),
                         dim3(256), 0, s, X, ldx, T, ldt, G, ldg, c_off, nc, nct);
    }, Ints<0, 1>{objective});
  };
  if (cs.n4 > 0) launch(f4{}, 0, cs.n4);
  if (cs.tail > 0) launch(float{}, cs.n4 * 4, cs.tail);
  return check_launch(nm);
}

int dol_mix_csr_pm_f32(const float* XT, int64_t ldx, int32_t x_rows, float* YT, int64_t ldy, int32_t n_rows,
                       int64_t P, const int32_t* rowptr, const int32_t* col, const float* val, hipStream_t s) {
  return dol_mix_csr_pm_ex_f32(XT, ldx, x_rows, YT, ldy, n_rows, P, rowptr, col, val, 0, s);
}

int dol_mix_csr_pm_ex_f32(const float* XT, int64_t ldx, int32_t x_rows, float* YT, int64_t ldy, int32_t n_rows,
                          int64_t P, const int32_t* rowptr, const int32_t* col, const float* val, int32_t nseg,
                          hipStream_t s) {
  DOL_DIMS_OK("dol_mix_csr_pm_f32", ldx, ldy, P);
  return mix_csr_pm_impl("dol_mix_csr_pm_f32", XT, ldx, x_rows, YT, ldy, n_rows, P, rowptr, col, val, -1, 0, PmDgd{},
                         nseg, s);
}

int dol_dgd_csr_pm_f32(const float* XT, int64_t ldx, int32_t x_rows, float* YT, int64_t ldy, int32_t n_rows,
                       int64_t P, const int32_t* rowptr, const int32_t* col, const float* val, const float* TT,
                       int64_t ldt, float* MT, int64_t ldm, int32_t objective, int32_t local_steps, float lr,
                       float momentum, int first_step, hipStream_t s) {
  return dol_dgd_csr_pm_ex_f32(XT, ldx, x_rows, YT, ldy, n_rows, P, rowptr, col, val, TT, ldt, MT, ldm, objective,
                               local_steps, lr, momentum, first_step, 0, s);
}

int dol_dgd_csr_pm_ex_f32(const float* XT, int64_t ldx, int32_t x_rows, float* YT, int64_t ldy, int32_t n_rows,
                          int64_t P, const int32_t* rowptr, const int32_t* col, const float* val, const float* TT,
                          int64_t ldt, float* MT, int64_t ldm, int32_t objective, int32_t local_steps, float lr,
                          float momentum, int first_step, int32_t nseg, hipStream_t s) {
  DOL_DIMS_OK("dol_dgd_csr_pm_f32", ldx, ldy, P, ldt, ldm);
  const char* nm = "dol_dgd_csr_pm_f32";
  if (objective != 0 && objective != 1) return fail(DOL_EINVAL, "%s: objective must be 0 or 1", nm);
  if (local_steps < 1) return fail(DOL_EINVAL, "%s: local_steps must be >= 1", nm);
  const int mode = momentum_mode(momentum, first_step);
  const PmDgd e{TT, ldt, mode ? MT : nullptr, mode ? ldm : 0, -lr, momentum, local_steps};
  return mix_csr_pm_impl(nm, XT, ldx, x_rows, YT, ldy, n_rows, P, rowptr, col, val, objective, mode, e, nseg, s);
}

int dol_mix_csr_pm_steps_f32(const float* XT, int64_t ldx, float* YT, int64_t ldy, int32_t n, int64_t P,
                             const int32_t* rowptr, const int32_t* col, const float* val, int32_t steps,
                             hipStream_t s) {
  return dol_mix_csr_pm_steps_ex_f32(XT, ldx, YT, ldy, n, P, rowptr, col, val, steps, 0, s);
}

int dol_mix_csr_pm_steps_ex_f32(const float* XT, int64_t ldx, float* YT, int64_t ldy, int32_t n, int64_t P,
                                const int32_t* rowptr, const int32_t* col, const float* val, int32_t steps,
                                int32_t nseg, hipStream_t s) {
  DOL_DIMS_OK("dol_mix_csr_pm_steps_f32", ldx, ldy, P);
  return mix_csr_pm_impl("dol_mix_csr_pm_steps_f32", XT, ldx, n, YT, ldy, n, P, rowptr, col, val, -1, 0, PmDgd{}, nseg,
                         s, steps);
}

int dol_dgd_csr_pm_steps_f32(const float* XT, int64_t ldx, float* YT, int64_t ldy, int32_t n, int64_t P,
                             const int32_t* rowptr, const int32_t* col, const float* val, const float* TT,
                             int64_t ldt, float* MT, int64_t ldm, int32_t objective, int32_t mix_steps,
                             int32_t local_steps, float lr, float momentum, int first_step, hipStream_t s) {
  return dol_dgd_csr_pm_steps_ex_f32(XT, ldx, YT, ldy, n, P, rowptr, col, val, TT, ldt, MT, ldm, objective, mix_steps,
                                     local_steps, lr, momentum, first_step, 0, s);
}

int dol_dgd_csr_pm_steps_ex_f32(const float* XT, int64_t ldx, float* YT, int64_t ldy, int32_t n, int64_t P,
                                const int32_t* rowptr, const int32_t* col, const float* val, const float* TT,
                                int64_t ldt, float* MT, int64_t ldm, int32_t objective, int32_t mix_steps,
                                int32_t local_steps, float lr, float momentum, int first_step, int32_t nseg,
                                hipStream_t s) {
  DOL_DIMS_OK("dol_dgd_csr_pm_steps_f32", ldx, ldy, P, ldt, ldm);
  const char* nm = "dol_dgd_csr_pm_steps_f32";
  if (objective != 0 && objective != 1) return fail(DOL_EINVAL, "%s: objective must be 0 or 1", nm);
  if (local_steps < 1) return fail(DOL_EINVAL, "%s: local_steps must be >= 1", nm);
  const int mode = momentum_mode(momentum, first_step);
  const PmDgd e{TT, ldt, mode ? MT : nullptr, mode ? ldm : 0, -lr, momentum, local_steps};
  return mix_csr_pm_impl(nm, XT, ldx, n, YT, ldy, n, P, rowptr, col, val, objective, mode, e, nseg, s, mix_steps);
}

int dol_transpose_f32(const float* A, int64_t lda, float* B, int64_t ldb, int64_t rows, int64_t cols, hipStream_t s) {
  DOL_DIMS_OK("dol_transpose_f32", lda, ldb, rows, cols);
  const char* nm = "dol_transpose_f32";
  if (rows < 0 || cols < 0) return fail(DOL_EINVAL, "%s: negative size", nm);
  if (rows == 0 || cols == 0) { dol::g_err[0] = '\0'; return DOL_OK; }
  if (!A || !B) return fail(DOL_EINVAL, "%s: null pointer", nm);
  if (lda < cols || ldb < rows) return fail(DOL_EINVAL, "%s: lda < cols or ldb < rows", nm);
  if (A == B) return fail(DOL_EINVAL, "%s: in-place transpose is not supported", nm);
  const int64_t tr = (rows + 63) / 64, tc = (cols + 63) / 64;
  if (tr * tc >= (int64_t(1) << 31)) return fail(DOL_EINVAL, "%s: too large", nm);
  hipLaunchKernelGGL(transpose_kernel, dim3(static_cast<unsigned>(tr * tc)), dim3(256), 0, s, A, lda, B, ldb, rows,
                     cols, tc);
  return check_launch(nm);
}

}  // extern "C"
