// CDNA4 (gfx950) kernels for SAE-ensemble training, fp32 end to end.
//
// These implement the reference's implicit kernel inventory (SURVEY.md §2.4
// K1-K6: encoder GEMM -> ReLU -> decoder GEMM -> MSE+L1 forward, analytic
// backward through the in-forward decoder row renormalization, fused Adam)
// as hand-written MFMA kernels.  fp32 is the reference's training dtype
// (BASELINE.md); we use the exact-f32 matrix instruction
// v_mfma_f32_32x32x2_f32 (157 TF peak, bitwise == an fmaf chain).
//
// GEMM core structure (tuned from rocprof on MI355X):
//  * 128x128 output tile, 8 waves (512 threads); each wave owns a 32x64
//    quadrant as 2 v_mfma_f32_32x32x2_f32 accumulators (32 AGPRs).
//  * K-tile depth TBK is a template parameter:
//      TBK=32, __launch_bounds__(512,4): 64-66 KB LDS, 2 blocks/CU.
//      TBK=16, __launch_bounds__(512,6): 32-33 KB LDS — more co-resident
//        blocks to hide barrier skew (SQ_WAIT_ANY was 25-33% of wave cycles
//        at 2 blocks/CU).  The bound asks for 3 blocks/CU; what runs follows
//        from the registers (an 8-wave block takes 2 wave slots per SIMD):
//        guarded enc, gc, gc_thresh and dec take 69-71 VGPRs = 7 waves/SIMD
//        = 3 blocks/CU; guarded grad_w, enc_fwd2 and gc2 take 60-62 and fit
//        4 blocks/CU (derived from the code object's metadata, not observed
//        on the device; per-kernel table: profiles/README.md, r04).
//    Both are compiled; the launcher picks at runtime (ops.kconfig).
//  * ALIGNED template flag: every GEMM kernel also exists without its row,
//    column and K-tail guards (plain float4 staging loads, unguarded epilogue
//    accesses through one scalar base + one 32-bit lane offset).  K-loop, MFMA
//    order and epilogue arithmetic are the guarded kernel's, so the outputs
//    are the same bit for bit.  The launchers (sae_ops.hip) take these on
//    tile-aligned shapes.  Without the guards the TBK=16 variants of enc, gc,
//    gc_thresh and grad_w fit __launch_bounds__(512,8): <= 64 VGPRs, no
//    scratch, 4 blocks/CU (tests/test_codeobject_occupancy.py holds them to
//    that); k_dec_fwd_t<16> would spill there and stays at (512,6).
//  * ping-pong LDS double buffer + register prefetch (guide T14/G15): ONE
//    barrier per K-step; the NEXT K-tile's global loads issue before the
//    MFMA phase of the current tile and are waited for (counted vmcnt) after
//    its last MFMA, in front of the LDS writes.  In the ALIGNED variants the
//    compiler does not keep that order by itself; gemm_mainloop says what pins
//    it, tests/test_codeobject_schedule.py checks every aligned variant's
//    loop in the built code object (table: profiles/README.md, r07).  The
//    guarded variants wait vmcnt(0) for their (conditional) loads before the
//    writes; the fragment reads of the MFMA phase are just-in-time (ds_read,
//    lgkmcnt(0), 2 MFMAs) in every variant.
//  * LDS staging is conflict-free: transposed tiles use stride BM+1 (b32
//    writes); direct tiles use stride BM with float4 (b128) writes.
//  * optional s_setprio(1) on the second-dispatched wave half (runtime
//    `prio` flag; MI355X_MICROARCH "Two waves per SIMD" item 4).
//  * XCD-aware bijective block swizzle (guide T1): consecutive remapped
//    blocks land on one XCD and share operand panels in its private L2.
//
// The seven GEMM kernels share one skeleton, written once as device functions:
//   Tile<TBN>            prologue: priority, model, swizzled tile, zeroed acc
//   TStage/TLds, DStage/DLds   one operand's registers in flight and its LDS
//                        buffers; the LDS type owns extent and stride
//   gemm_mainloop        the prefetch K-loop; the kernel passes its two loads
//                        and two LDS writes as lambdas (k_gc_t alone writes
//                        the loop out: measured slower through the function)
//   epi_cols / epi_rows  the epilogue's walk over the accumulators, with the
//                        guards and the element accessor `at` (k_gc_t and
//                        k_gc_thresh_t write the same walk out: the helpers
//                        cost their 8-waves/SIMD variants a register and time)
//   halfwave_pair_sum    per-column sum across the two half-waves
// A kernel body holds its operand pointers, its four staging lambdas and its
// per-element / per-column epilogue arithmetic.  The epilogues switch
// floating-point contraction off (k_enc_fwd2_t/k_gc2_t excepted: guarded only).
//
// Kernels (each a template over TBK, MINW, TBN, ALIGNED):
//   k_enc_fwd_t  : c = relu(x @ Wenc^T + b)    (+ L1 partial, fired counts)
//   k_enc_fwd2_t : same with pre-transposed operands (all-direct staging)
//   k_dec_fwd_t  : r = c @ Wdec_hat - x        (+ MSE partial)
//   k_gc_t/k_gc2_t: gpre = (c>0) .* (gs * r @ Wdec_hat^T + l1/B) (+ bias-grad;
//                  k_gc_t stores per-32-row column sums, k_colsum_groups adds
//                  them in a fixed order: reproducible; k_gc2_t uses atomics)
//   k_grad_w_t   : gw = beta*gw + alpha * P^T @ Q   (K = batch contraction)
//   k_row_norms, k_project_adam (gradient of w/max(||w||,eps)), k_bias_adam,
//   k_transpose_scale, k_colsum (HBM-rate column sums / L1 reductions),
//   k_topk_select (exact per-row radix top-k), k_btk_hist/k_btk_write (exact
//   batch-level radix top-k over many workgroups), k_resample (K14 on-device),
//   k_lista_bwd_elem (one-pass LISTA backward elementwise chain)

#include <hip/hip_runtime.h>

#include <type_traits>

#define WAVE 64
#define BM 128
#define BN 128
#define NTHREADS 512
#define NXCD 8

typedef float f32x16 __attribute__((ext_vector_type(16)));

// C/D fragment mapping for 32x32 MFMA (guide §3): reg r, lane l ->
//   row = (r&3) + 8*(r>>2) + 4*(l>>5), col = l&31
__device__ __forceinline__ int acc_row(int r, int lane) {
  return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
}

// Bijective XCD-contiguous remap of a linear block id (guide T1; bijective
// variant for nwg % 8 != 0).
__device__ __forceinline__ long xcd_swizzle(long id, long nwg) {
  long q = nwg / NXCD, r = nwg % NXCD;
  long xcd = id % NXCD, pos = id / NXCD;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + pos;
}

// Decompose blockIdx (x = col tile, y = row tile, z = model) after swizzling
// the (x, y) plane per model so that co-XCD blocks share operand panels.
__device__ __forceinline__ void tile_coords(int& tx, int& ty) {
  long nwg = (long)gridDim.x * gridDim.y;
  long id = (long)blockIdx.x + (long)gridDim.x * blockIdx.y;
  long s = xcd_swizzle(id, nwg);
  tx = (int)(s % gridDim.x);
  ty = (int)(s / gridDim.x);
}

// Optional static priority for the second-dispatched wave half: the younger
// waves lose VALU arbitration on every segment; one setprio before the main
// loop, no per-segment flips.
__device__ __forceinline__ void maybe_prio(int prio) {
  if (prio && threadIdx.x >= NTHREADS / 2) __builtin_amdgcn_s_setprio(1);
}

// ---------------------------------------------------------------------------
// staging: load (global -> regs) and write (regs -> LDS) split so the loads
// overlap the previous tile's MFMA phase.  TBK/16 float4 passes per thread.
// ---------------------------------------------------------------------------

// Each operand layout comes as a pair: the registers of one tile in flight
// (TStage/DStage) and its ping-pong LDS buffers (TLds/DLds).  The LDS type owns
// the extent and the row stride; stage_*_write accepts only the matching type
// and mfma_tile reads STRIDE from it, so a kernel states a layout once, in its
// __shared__ declaration, and the three cannot disagree.

// Transposed tile: lds[k][i] = src[i0+i][k0+k] (* scale[i0+i]), i<TROWS, k<TBK.
template <int TBK, int TROWS = BM>
struct TStage {
  float4 v[TBK * TROWS / 2048];
  float sc[TBK * TROWS / 2048];
};
template <int TBK, int TROWS = BM>
struct TLds {
  static constexpr int STRIDE = TROWS + 1;  // padded: conflict-free b32 writes
  float buf[2][TBK * STRIDE];
};

// ALIGNED: the caller guarantees a full tile (no row or K tail) and 16-byte
// aligned rows, so every load is one unguarded float4.
template <int TBK, int TROWS = BM, bool ALIGNED = false>
__device__ __forceinline__ void stage_T_load(const float* __restrict__ src, long ld,
                                             int i0, int k0, int n_rows, int n_k,
                                             TStage<TBK, TROWS>& st) {
  const int t = threadIdx.x;
  constexpr int TPR = TBK / 4;                 // threads covering one row's K
  constexpr int RPP = NTHREADS / TPR;          // rows per pass
#pragma unroll
  for (int p = 0; p < TBK * TROWS / 2048; ++p) {
    int i = p * RPP + t / TPR;
    int kc = (t % TPR) * 4;
    int gi = i0 + i;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (ALIGNED) {
      v = *reinterpret_cast<const float4*>(src + (long)gi * ld + k0 + kc);
    } else if (gi < n_rows) {
      const float* row = src + (long)gi * ld + k0 + kc;
      if (k0 + kc + 3 < n_k) {
        v = *reinterpret_cast<const float4*>(row);
      } else {
#pragma unroll
        for (int s = 0; s < 4; ++s)
          if (k0 + kc + s < n_k) ((float*)&v)[s] = row[s];
      }
    }
    st.v[p] = v;
  }
}

// The scale of a transposed tile belongs to its row, not to the K-tile, so it
// is loaded once, ahead of the K-loop (1 where there is no scale or no row).
// Loaded with every tile, it sat at the top of the unguarded gc kernels' MFMA
// phase with a vmcnt(0) behind it that also waited for the tile loads.
template <int TBK, int TROWS, bool ALIGNED>
__device__ __forceinline__ void stage_T_scale(const float* __restrict__ scale, int i0, int n_rows,
                                              TStage<TBK, TROWS>& st) {
  constexpr int RPP = NTHREADS / (TBK / 4);
#pragma unroll
  for (int p = 0; p < TBK * TROWS / 2048; ++p) {
    int gi = i0 + p * RPP + threadIdx.x / (TBK / 4);
    st.sc[p] = (scale && (ALIGNED || gi < n_rows)) ? scale[gi] : 1.f;
  }
}

template <int TBK, int TROWS>
__device__ __forceinline__ void stage_T_write(const TStage<TBK, TROWS>& st, TLds<TBK, TROWS>& dst,
                                              int buf, bool scaled) {
  float* __restrict__ lds = dst.buf[buf];
  const int t = threadIdx.x;
  constexpr int TPR = TBK / 4;
  constexpr int RPP = NTHREADS / TPR;
#pragma unroll
  for (int p = 0; p < TBK * TROWS / 2048; ++p) {
    int i = p * RPP + t / TPR;
    int kc = (t % TPR) * 4;
    float4 v = st.v[p];
    if (scaled) {
      v.x *= st.sc[p]; v.y *= st.sc[p]; v.z *= st.sc[p]; v.w *= st.sc[p];
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) lds[(kc + s) * TLds<TBK, TROWS>::STRIDE + i] = ((float*)&v)[s];
  }
}

// Direct tile: lds[k][j] = src[k0+k][j0+j] (* scale[k0+k]), k<TBK, j<TCOLS.
template <int TBK, int TCOLS = BM>
struct DStage {
  float4 v[TBK * TCOLS / 2048];
  float sc[TBK * TCOLS / 2048];
};
template <int TBK, int TCOLS = BM>
struct DLds {
  static constexpr int STRIDE = TCOLS;  // float4 (b128) writes
  float buf[2][TBK * STRIDE];
};

template <int TBK, int TCOLS = BM, bool ALIGNED = false>
__device__ __forceinline__ void stage_D_load(const float* __restrict__ src, long ld,
                                             int k0, int j0, int n_k, int n_cols,
                                             const float* __restrict__ scale,
                                             DStage<TBK, TCOLS>& st) {
  const int t = threadIdx.x;
  constexpr int TPC = TCOLS / 4;               // threads covering one k's cols
  constexpr int KPP = NTHREADS / TPC;          // k rows per pass
#pragma unroll
  for (int p = 0; p < TBK * TCOLS / 2048; ++p) {
    int k = p * KPP + t / TPC;
    int j = (t % TPC) * 4;
    int gk = k0 + k;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    float sc = 1.f;
    if constexpr (ALIGNED) {
      v = *reinterpret_cast<const float4*>(src + (long)gk * ld + j0 + j);
      if (scale) sc = scale[gk];
    } else if (gk < n_k) {
      const float* row = src + (long)gk * ld + j0 + j;
      if (j0 + j + 3 < n_cols) {
        v = *reinterpret_cast<const float4*>(row);
      } else {
#pragma unroll
        for (int s = 0; s < 4; ++s)
          if (j0 + j + s < n_cols) ((float*)&v)[s] = row[s];
      }
      if (scale) sc = scale[gk];
    }
    st.v[p] = v;
    st.sc[p] = sc;
  }
}

template <int TBK, int TCOLS>
__device__ __forceinline__ void stage_D_write(const DStage<TBK, TCOLS>& st, DLds<TBK, TCOLS>& dst,
                                              int buf, bool scaled) {
  float* __restrict__ lds = dst.buf[buf];
  const int t = threadIdx.x;
  constexpr int TPC = TCOLS / 4;
  constexpr int KPP = NTHREADS / TPC;
#pragma unroll
  for (int p = 0; p < TBK * TCOLS / 2048; ++p) {
    int k = p * KPP + t / TPC;
    int j = (t % TPC) * 4;
    float4 v = st.v[p];
    if (scaled) {
      v.x *= st.sc[p]; v.y *= st.sc[p]; v.z *= st.sc[p]; v.w *= st.sc[p];
    }
    *reinterpret_cast<float4*>(&lds[k * DLds<TBK, TCOLS>::STRIDE + j]) = v;
  }
}

// ---------------------------------------------------------------------------
// MFMA phase: 8 waves; wave w covers rows [(w&3)*32, +32), cols [(w>>2)*64, +64)
// ---------------------------------------------------------------------------
template <int TBK, int NACC, int ASTRIDE, int BSTRIDE>
__device__ __forceinline__ void mfma_tile(const float* __restrict__ As,
                                          const float* __restrict__ Bs,
                                          f32x16 (&acc)[NACC]) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  const int wr = (wave & 3) * 32;
  const int wc = (wave >> 2) * (NACC * 32);
  const int l31 = lane & 31;
  const int h = lane >> 5;

#pragma unroll
  for (int kk = 0; kk < TBK; kk += 2) {
    float a0 = As[(kk + h) * ASTRIDE + wr + l31];
#pragma unroll
    for (int j = 0; j < NACC; ++j) {
      float b = Bs[(kk + h) * BSTRIDE + wc + j * 32 + l31];
      acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b, acc[j], 0, 0, 0);
    }
  }
}

// Ping-pong double buffer + register prefetch: ONE barrier per K-step.
// Iteration t: issue loads of tile t+1, MFMA on buffer `cur` (tile t), write
// tile t+1 into buffer cur^1 (nobody reads it), barrier, flip.  The barrier
// at the end of iteration t also protects the write of tile t+2 into the
// old `cur` (every wave has finished reading it).
// load_a/load_b(k0) fetch the K-tile at k0 into the kernel's stage registers,
// write_a/write_b(buf) store those registers into LDS buffer `buf`.
// k_gc_t holds a written-out copy of this loop (the reason is stated there):
// a change to the order of operations here has to be made there too.
//
// The order above is the source's; two things pin it in the code object
// (tests/test_codeobject_schedule.py reads it back from the disassembly):
//  * kloop_loads_issued(): an unguarded load of a `const __restrict__` kernel
//    argument is a load of constant memory to the compiler, free of any
//    ordering, and instruction selection sinks it to its first use: behind the
//    MFMA phase, straight in front of its own s_waitcnt.  The staged operands
//    of the GEMM kernels are therefore NOT declared __restrict__, and the
//    compiler-only memory fence after the loads keeps them ahead of the LDS
//    reads of the MFMA phase.  Either alone changes nothing.  It is the
//    qualifier on the KERNEL's arguments that matters: the `__restrict__` on
//    the `src` parameter of stage_T_load / stage_D_load is inlined away and
//    does no harm; do not put it back on the kernels to match.
//  * kloop_mfma_issued(): a scheduling barrier between the MFMA phase and the
//    LDS writes.  Without it the scheduler pulls the writes' scale multiplies
//    in among the first MFMAs, and the s_waitcnt vmcnt they need with them.
//    Mask 0x8: MFMAs alone may cross it, so the last one or two still run
//    behind the writes and the workgroup barrier (with mask 0 the TBK=32
//    k_dec_fwd_t measured 10 us slower; profiles/README.md, r07).
__device__ __forceinline__ void kloop_loads_issued() { asm volatile("" ::: "memory"); }
__device__ __forceinline__ void kloop_mfma_issued() { __builtin_amdgcn_sched_barrier(0x8); }

template <int TBK, int NACC, class ALds, class BLds, class LoadA, class LoadB, class WriteA,
          class WriteB>
__device__ __forceinline__ void gemm_mainloop(int k_total, ALds& As, BLds& Bs, f32x16 (&acc)[NACC],
                                              LoadA load_a, LoadB load_b, WriteA write_a,
                                              WriteB write_b) {
  constexpr int ASTR = ALds::STRIDE, BSTR = BLds::STRIDE;
  int cur = 0;
  load_a(0);
  load_b(0);
  write_a(0);
  write_b(0);
  __syncthreads();
  for (int k0 = TBK; k0 < k_total; k0 += TBK) {
    load_a(k0);
    load_b(k0);
    kloop_loads_issued();
    mfma_tile<TBK, NACC, ASTR, BSTR>(As.buf[cur], Bs.buf[cur], acc);
    kloop_mfma_issued();
    write_a(cur ^ 1);
    write_b(cur ^ 1);
    __syncthreads();
    cur ^= 1;
  }
  mfma_tile<TBK, NACC, ASTR, BSTR>(As.buf[cur], Bs.buf[cur], acc);
}

// Where a GEMM kernel starts: wave priority, this block's model and (swizzled)
// output tile, and the zeroed accumulators of a BM x TBN tile.
template <int TBN>
struct Tile {
  static constexpr int NACC = TBN / 64;
  int m, row0, col0;
  f32x16 acc[NACC];
  __device__ __forceinline__ explicit Tile(int prio) {
    maybe_prio(prio);
    m = blockIdx.z;
    int tx, ty;
    tile_coords(tx, ty);
    row0 = ty * BM;
    col0 = tx * TBN;
#pragma unroll
    for (int j = 0; j < NACC; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  }
};

__device__ __forceinline__ float wave_reduce_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
  return v;
}

// epilogue lane geometry shared by all GEMM kernels
struct EpiGeom {
  int lane, wave, wr, wc, l31;
};
template <int NACC = 2>
__device__ __forceinline__ EpiGeom epi_geom() {
  EpiGeom g;
  g.lane = threadIdx.x & (WAVE - 1);
  g.wave = threadIdx.x / WAVE;
  g.wr = (g.wave & 3) * 32;
  g.wc = (g.wave >> 2) * (NACC * 32);
  g.l31 = g.lane & 31;
  return g;
}

// Index of accumulator element (tj, r) in a row-major [rows, ld] epilogue
// operand.  The guarded kernels form it per element from (row, col).  ALIGNED
// splits it into a block-uniform 64-bit part, which lives in scalar registers,
// and one 32-bit offset per lane, so the 32 accesses of a thread share one
// address VGPR instead of holding a 64-bit pair each (the launchers admit
// ld < 2^23 only, so the lane part cannot wrap).
template <bool ALIGNED>
struct EpiIndex {
  long tile;
  unsigned lane_off;  // bytes
  int ld;
  __device__ __forceinline__ EpiIndex(int row0, int col0, int ld_, const EpiGeom& g) : ld(ld_) {
    // row0/col0 are block-uniform but come out of a 64-bit division done in
    // vector registers; readfirstlane moves them (and `tile`) to scalar ones
    tile = (long)__builtin_amdgcn_readfirstlane(row0) * ld + __builtin_amdgcn_readfirstlane(col0);
    lane_off = 4u * (unsigned)((g.wr + 4 * (g.lane >> 5)) * ld + g.wc + g.l31);
  }
  template <typename T>
  __device__ __forceinline__ T& ref(T* base, int row, int col, int r, int tj) {
    if constexpr (ALIGNED) {
      T* pu = base + (tile + (long)((r & 3) + 8 * (r >> 2)) * ld + tj * 32);
      // make lane_off opaque at every access (in place, no instruction):
      // otherwise the compiler hoists base + lane_off into a 64-bit VGPR
      // pointer and steps that per row
      asm volatile("" : "+v"(lane_off));
      using B = std::conditional_t<std::is_const_v<T>, const char, char>;
      return *reinterpret_cast<T*>(reinterpret_cast<B*>(pu) + lane_off);
    } else {
      return base[(long)row * ld + col];
    }
  }
};

// The epilogue's walk over a thread's accumulators, shared by the GEMM kernels
// (k_gc_t and k_gc_thresh_t write it out, see there): NACC column blocks (one
// column per lane each), 16 rows per block.
// A kernel's epilogue is per_col(tj, col, col_ok) holding its per-column head
// and tail around one epi_rows call; per_elem(r, at) runs for the in-range
// elements, with at(p) the element's slot in a row-major [rows, ld] operand.
// A `#pragma clang fp contract(off)` at the top of a per_col lambda reaches
// the lambdas defined inside it (checked on the ISA: mul + add, no fma).
template <int NACC, bool ALIGNED, class PerCol>
__device__ __forceinline__ void epi_cols(const EpiGeom& g, int col0, int n_cols, PerCol per_col) {
#pragma unroll
  for (int tj = 0; tj < NACC; ++tj) {
    int col = col0 + g.wc + tj * 32 + g.l31;
    per_col(tj, col, ALIGNED || col < n_cols);
  }
}

template <bool ALIGNED, class PerElem>
__device__ __forceinline__ void epi_rows(const EpiGeom& g, EpiIndex<ALIGNED>& ei, int row0,
                                         int n_rows, int tj, int col, bool col_ok,
                                         PerElem per_elem) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    int row = row0 + g.wr + acc_row(r, g.lane);
    if ((ALIGNED || row < n_rows) && col_ok)
      per_elem(r, [&](auto* p) -> auto& { return ei.ref(p, row, col, r, tj); });
  }
}

// A column of a wave's 32x32 block lives in lanes l and l+32 (rows 4h..4h+3 of
// every 8, h = lane>>5).  tot = this lane's partial + the other half-wave's;
// true for the lane that owns the column's store or atomic (lane < 32).
__device__ __forceinline__ bool halfwave_pair_sum(const EpiGeom& g, float v, float& tot) {
  float other = __shfl_xor(v, 32, WAVE);
  tot = v + other;
  return g.lane < 32;
}

// ---------------------------------------------------------------------------
// k_row_norms
// ---------------------------------------------------------------------------
extern "C" __global__ void k_row_norms(const float* __restrict__ W,
                                       float* __restrict__ norms,
                                       float* __restrict__ inv_norms,
                                       int n_rows_total, int d, float eps) {
  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int row = blockIdx.x * (NTHREADS / WAVE) + wave;
  if (row >= n_rows_total) return;
  const float* w = W + (long)row * d;
  float s = 0.f;
  if (d % (WAVE * 4) == 0) {
    for (int j = lane * 4; j < d; j += WAVE * 4) {
      float4 v = *reinterpret_cast<const float4*>(w + j);
      s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    }
  } else {
    for (int j = lane; j < d; j += WAVE) s += w[j] * w[j];
  }
  s = wave_reduce_sum(s);
  if (lane == 0) {
    float nrm = sqrtf(s);
    norms[row] = nrm;
    inv_norms[row] = 1.0f / fmaxf(nrm, eps);
  }
}

// Epilogue selectors of k_enc_fwd_t/k_enc_fwd2_t (`mode`) and k_gc_t/k_gc2_t
// (`gc_mode`); the values are the integers the Python side passes.
enum EncMode : int {
  ENC_RELU = 0,       // c = relu(acc + b), masked by dict_sizes (+L1, fired)
  ENC_RAW = 1,        // raw scores for TopK selection
  ENC_GATE = 2,       // thresholding SAE's soft gate (+L1, fired, u)
  ENC_REVERSE = 3,    // reverse SAE: c = acc * [acc + b > 0] (+L1, fired)
  ENC_LISTA_FWD = 4,  // LISTA layer: shrink + momentum
  ENC_LISTA_BWD = 5,  // LISTA backward: c = y_in - acc
};
enum GcMode : int {
  GC_RELU = 0,     // active set c > 0, bias gradient produced
  GC_REVERSE = 1,  // reverse SAE: active set c != 0, sign(c) l1 term, no bias grad
};

// The soft-threshold gate of the thresholding SAE (reference
// sae_ensemble.py:256-259): u = (c + gain) / max(a^2, eps),
// g(u) = relu6(60(u-0.9))/6 + relu(u-1), code = g(u) * a^2 (RAW a^2 — the
// reference multiplies by the unclamped square).
// Floating-point contraction is switched off in the epilogues below and every
// fused multiply-add is written out: the guarded and the ALIGNED variant of a
// kernel then round alike whatever the optimiser makes of either (left to
// itself it fuses differently once the guards are gone).  The fmaf calls are
// the contractions the guarded kernels were compiled with.
#define GATE_EPS 1e-8f
__device__ __forceinline__ float gate_g(float u) {
#pragma clang fp contract(off)
  return fmaf(fminf(fmaxf(60.0f * (u - 0.9f), 0.0f), 6.0f), 1.0f / 6.0f,
              fmaxf(u - 1.0f, 0.0f));
}
// g(x * s_inv) with the product folded into both subtractions (one rounding
// each instead of two): the encoder epilogue's form
__device__ __forceinline__ float gate_g_scaled(float x, float s_inv) {
#pragma clang fp contract(off)
  return fmaf(fminf(fmaxf(60.0f * fmaf(x, s_inv, -0.9f), 0.0f), 6.0f), 1.0f / 6.0f,
              fmaxf(fmaf(x, s_inv, -1.0f), 0.0f));
}
__device__ __forceinline__ float gate_gp(float u) {  // dg/du (0 at the kinks)
  float gp = (u > 0.9f && u < 1.0f) ? 10.0f : 0.0f;
  if (u > 1.0f) gp += 1.0f;
  return gp;
}

// ---------------------------------------------------------------------------
// k_enc_fwd_t
// ---------------------------------------------------------------------------
template <int TBK, int MINW, int TBN = BN, bool ALIGNED = false>
__global__ __launch_bounds__(NTHREADS, MINW)
void k_enc_fwd_t(const float* x,                    // [B, d]     (staged operands: no
                 const float* Wenc,                 // [M, n, d]   __restrict__, see gemm_mainloop)
                 const float* __restrict__ bias,    // [M, n]
                 const float* __restrict__ inv_norms, // [M, n] or nullptr
                 float* __restrict__ c_out,         // [M, B, n]
                 float* __restrict__ loss_parts,    // [M, 2]
                 float* __restrict__ fired,         // [M, n]
                 int B, int d, int n,
                 int mode,  // an EncMode
                 int prio,
                 const float* __restrict__ act_scale,  // [M, n] (mode 2)
                 const float* __restrict__ act_gain,   // [M, n] (mode 2)
                 float* __restrict__ u_out,            // [M, B, n] (mode 2/4)
                 const int* __restrict__ dict_sizes, // [M] or nullptr:
                                       // masked sigs zero cols >= dict_sizes[m]
                 long x_mstride,       // 0: x shared [B,d]; else x is [M,B,d]
                 const float* __restrict__ y_in,   // [M, B, n] (modes 4, 5)
                 const float* __restrict__ x_prev, // [M, B, n] (mode 4)
                 float* __restrict__ x_out,        // [M, B, n] (mode 4)
                 const float* __restrict__ mom) {  // [M] momentum (mode 4)
  __shared__ TLds<TBK, BM> As;
  __shared__ TLds<TBK, TBN> Bs;

  constexpr int NACC = Tile<TBN>::NACC;
  Tile<TBN> t(prio);
  const int m = t.m;
  const float* W = Wenc + (long)m * n * d;
  const float* x_m = x + (long)m * x_mstride;
  const float* inv = inv_norms ? inv_norms + (long)m * n : nullptr;
  const bool scaled = inv != nullptr;

  TStage<TBK, BM> sa;
  TStage<TBK, TBN> sb;
  stage_T_scale<TBK, TBN, ALIGNED>(inv, t.col0, n, sb);
  gemm_mainloop<TBK>(
      d, As, Bs, t.acc,
      [&](int k0) { stage_T_load<TBK, BM, ALIGNED>(x_m, d, t.row0, k0, B, d, sa); },
      [&](int k0) { stage_T_load<TBK, TBN, ALIGNED>(W, d, t.col0, k0, n, d, sb); },
      [&](int buf) { stage_T_write(sa, As, buf, false); },
      [&](int buf) { stage_T_write(sb, Bs, buf, scaled); });

  const EpiGeom g = epi_geom<NACC>();
  EpiIndex<ALIGNED> ei(t.row0, t.col0, n, g);
  float* c_m = c_out + (long)m * B * n;
  const float* bias_m = bias + (long)m * n;
  float* fired_m = fired + (long)m * n;

  float l1_sum = 0.f;
  epi_cols<NACC, ALIGNED>(g, t.col0, n, [&](int tj, int col, bool col_ok) {
#pragma clang fp contract(off)
    const f32x16& acc = t.acc[tj];
    auto rows = [&](auto per_elem) {
      epi_rows<ALIGNED>(g, ei, t.row0, B, tj, col, col_ok, per_elem);
    };
    // fired[m, col] += the wave's count of active rows in this column
    auto add_fired = [&](float fired_cnt) {
      float tot;
      if (col_ok && halfwave_pair_sum(g, fired_cnt, tot) && tot > 0.f)
        atomicAdd(&fired_m[col], tot);
    };
    if (mode == ENC_RAW) {
      // raw scores for TopK selection: no bias, no relu, no side outputs
      rows([&](int r, auto at) { at(c_m) = acc[r]; });
    } else if (mode == ENC_GATE) {
      // thresholding SAE: code = g((c+gain)/max(a^2,eps)) * a^2; u kept for
      // the backward's gate derivative (k_gc_thresh_t)
      float a = col_ok ? act_scale[(long)m * n + col] : 1.f;
      float gn = col_ok ? act_gain[(long)m * n + col] : 0.f;
      float s_raw = a * a;
      float s_inv = 1.0f / fmaxf(s_raw, GATE_EPS);
      float* u_m = u_out + (long)m * B * n;
      float fired_cnt = 0.f;
      rows([&](int r, auto at) {
        float av = acc[r];
        // unguarded, the 16 gate chains of a column would be vectorised
        // side by side, past the 64 registers of 8 waves/SIMD; an opaque
        // accumulator value keeps them one after the other
        if constexpr (ALIGNED) asm volatile("" : "+v"(av));
        float u = (av + gn) * s_inv;
        float code = gate_g_scaled(av + gn, s_inv) * s_raw;
        at(c_m) = code;
        at(u_m) = u;
        l1_sum += code;
        fired_cnt += (code > 0.f) ? 1.f : 0.f;
      });
      add_fired(fired_cnt);
    } else if (mode == ENC_LISTA_FWD || mode == ENC_LISTA_BWD) {
      // LISTA layer epilogues (HipLISTAStep): the GEMM result `acc` is
      //   mode 4:  s = neg_e W_l^T;  r = y - s;  x = shrink(r, theta);
      //            y' = x + m (x - x_prev)   -> u_out=r, x_out=x, c_out=y'
      //   mode 5:  c_out = y_in - acc        (backward g_y = g_r - g_e A^T)
      const float* y_m = y_in + (long)m * (long)B * n;
      float th = 0.f, mm = 0.f;
      const float* xp_m = nullptr;
      float* xo_m = nullptr;
      float* u_m = nullptr;
      if (mode == ENC_LISTA_FWD) {
        th = col_ok ? act_scale[(long)m * n + col] : 0.f;
        mm = mom[m];
        xp_m = x_prev + (long)m * (long)B * n;
        xo_m = x_out + (long)m * (long)B * n;
        u_m = u_out + (long)m * (long)B * n;
      }
      rows([&](int r, auto at) {
        float v = at(y_m) - acc[r];
        if (mode == ENC_LISTA_BWD) {
          at(c_m) = v;
        } else {
          at(u_m) = v;  // r_l, kept for the backward's shrink mask
          float a = fabsf(v) - th;
          float xa = (a > 0.f) ? ((v > 0.f) ? a : -a) : 0.f;
          at(xo_m) = xa;
          at(c_m) = fmaf(mm, xa - at(xp_m), xa);
        }
      });
    } else if (mode == ENC_REVERSE) {
      // reverse SAE (sae_ensemble.py:447-503): code = pre * [pre + b > 0]
      // (the bias is removed from active features before decoding, so the
      // code can be negative and the L1 partial needs |code|)
      float bj = col_ok ? bias_m[col] : 0.f;
      float fired_cnt = 0.f;
      rows([&](int r, auto at) {
        float pre = acc[r];
        float v = (pre + bj > 0.f) ? pre : 0.f;
        at(c_m) = v;
        l1_sum += fabsf(v);
        fired_cnt += (v != 0.f) ? 1.f : 0.f;
      });
      add_fired(fired_cnt);
    } else {  // ENC_RELU
      float bj = col_ok ? bias_m[col] : 0.f;
      // coefficient mask (reference K9): columns >= dict_sizes[m] are dead
      bool live = col_ok && (!dict_sizes || col < dict_sizes[m]);
      float fired_cnt = 0.f;
      rows([&](int r, auto at) {
        float v = live ? fmaxf(acc[r] + bj, 0.f) : 0.f;
        at(c_m) = v;
        l1_sum += v;
        fired_cnt += (v > 0.f) ? 1.f : 0.f;
      });
      add_fired(fired_cnt);
    }
  });
  if (mode == ENC_RELU || mode == ENC_GATE || mode == ENC_REVERSE) {
    l1_sum = wave_reduce_sum(l1_sum);
    if (g.lane == 0) atomicAdd(&loss_parts[m * 2 + 1], l1_sum);
  }
}

// ---------------------------------------------------------------------------
// k_dec_fwd_t
// ---------------------------------------------------------------------------
template <int TBK, int MINW, int TBN = BN, bool ALIGNED = false>
__global__ __launch_bounds__(NTHREADS, MINW)
void k_dec_fwd_t(const float* c,                    // [M, B, n]  (staged operands: no
                 const float* Wdec,                 // [M, n, d]   __restrict__, see gemm_mainloop)
                 const float* __restrict__ inv_norms, // [M, n]
                 const float* __restrict__ x,       // [B, d]
                 float* __restrict__ r_out,         // [M, B, d]
                 float* __restrict__ loss_parts,    // [M, 2]
                 int B, int d, int n, int prio,
                 long x_mstride) {  // 0: shared [B,d]; else [M,B,d]
  __shared__ TLds<TBK, BM> As;
  __shared__ DLds<TBK, TBN> Bs;

  constexpr int NACC = Tile<TBN>::NACC;
  Tile<TBN> t(prio);
  const int m = t.m;
  const float* c_m = c + (long)m * B * n;
  const float* W = Wdec + (long)m * n * d;
  const float* x_m = x + (long)m * x_mstride;
  const float* inv = inv_norms + (long)m * n;

  TStage<TBK, BM> sa;
  DStage<TBK, TBN> sb;
  gemm_mainloop<TBK>(
      n, As, Bs, t.acc,
      [&](int k0) { stage_T_load<TBK, BM, ALIGNED>(c_m, n, t.row0, k0, B, n, sa); },
      [&](int k0) { stage_D_load<TBK, TBN, ALIGNED>(W, d, k0, t.col0, n, d, inv, sb); },
      [&](int buf) { stage_T_write(sa, As, buf, false); },
      [&](int buf) { stage_D_write(sb, Bs, buf, true); });

  const EpiGeom g = epi_geom<NACC>();
  EpiIndex<ALIGNED> ei(t.row0, t.col0, d, g);
  float* r_m = r_out + (long)m * B * d;

  float mse_sum = 0.f;
  epi_cols<NACC, ALIGNED>(g, t.col0, d, [&](int tj, int col, bool col_ok) {
#pragma clang fp contract(off)
    epi_rows<ALIGNED>(g, ei, t.row0, B, tj, col, col_ok, [&](int r, auto at) {
      float rv = t.acc[tj][r] - at(x_m);
      at(r_m) = rv;
      mse_sum = fmaf(rv, rv, mse_sum);
    });
  });
  mse_sum = wave_reduce_sum(mse_sum);
  if (g.lane == 0) atomicAdd(&loss_parts[m * 2 + 0], mse_sum);
}

// ---------------------------------------------------------------------------
// k_gc_t
// ---------------------------------------------------------------------------
template <int TBK, int MINW, int TBN = BN, bool ALIGNED = false>
__global__ __launch_bounds__(NTHREADS, MINW)
void k_gc_t(const float* r,                     // [M, B, d]  (staged operands: no
            const float* Wdec,                  // [M, n, d]   __restrict__, see gemm_mainloop)
            const float* __restrict__ inv_norms,// [M, n]
            const float* __restrict__ c,        // [M, B, n]
            const float* __restrict__ l1_alpha, // [M]
            float* __restrict__ gpre_out,       // [M, B, n]
            float* __restrict__ gb_part,        // [M, nrg, n] per-32-row column sums
            int B, int d, int n, int prio, int gc_mode) {
  __shared__ TLds<TBK, BM> As;
  __shared__ TLds<TBK, TBN> Bs;

  constexpr int NACC = Tile<TBN>::NACC;
  Tile<TBN> t(prio);
  const int m = t.m;
  const float* r_m = r + (long)m * B * d;
  const float* W = Wdec + (long)m * n * d;
  const float* inv = inv_norms + (long)m * n;
  const float* c_m = c + (long)m * B * n;
  const float gscale = 2.0f / ((float)B * (float)d);
  const float l1_term = l1_alpha[m] / (float)B;

  TStage<TBK, BM> sa;
  TStage<TBK, TBN> sb;
  // This kernel alone writes gemm_mainloop's loop and the epilogue walk out.
  // Through the helpers its aligned <16, 8, 128> variant is scheduled
  // differently (and with epi_cols/epi_rows takes 64 VGPRs, not 63) and
  // measured 0.4-0.7% slower (profiles/README.md, r04; that was before the
  // K-loop's order was pinned in r07 and has not been measured again since).
  {
    constexpr int ASTR = TLds<TBK, BM>::STRIDE, BSTR = TLds<TBK, TBN>::STRIDE;
    int cur = 0;
    stage_T_scale<TBK, TBN, ALIGNED>(inv, t.col0, n, sb);
    stage_T_load<TBK, BM, ALIGNED>(r_m, d, t.row0, 0, B, d, sa);
    stage_T_load<TBK, TBN, ALIGNED>(W, d, t.col0, 0, n, d, sb);
    stage_T_write(sa, As, 0, false);
    stage_T_write(sb, Bs, 0, true);
    __syncthreads();
    for (int k0 = TBK; k0 < d; k0 += TBK) {
      stage_T_load<TBK, BM, ALIGNED>(r_m, d, t.row0, k0, B, d, sa);
      stage_T_load<TBK, TBN, ALIGNED>(W, d, t.col0, k0, n, d, sb);
      kloop_loads_issued();
      mfma_tile<TBK, NACC, ASTR, BSTR>(As.buf[cur], Bs.buf[cur], t.acc);
      kloop_mfma_issued();
      stage_T_write(sa, As, cur ^ 1, false);
      stage_T_write(sb, Bs, cur ^ 1, true);
      __syncthreads();
      cur ^= 1;
    }
    mfma_tile<TBK, NACC, ASTR, BSTR>(As.buf[cur], Bs.buf[cur], t.acc);
  }

  const EpiGeom g = epi_geom<NACC>();
  EpiIndex<ALIGNED> ei(t.row0, t.col0, n, g);
  float* g_m = gpre_out + (long)m * B * n;
  // bias grad: each wave owns one 32-row group of its columns and stores that
  // group's column sum with a plain store; k_colsum_groups adds the groups in
  // a fixed order (bitwise reproducible, unlike float atomics across blocks)
  const int nrg = (B + 31) / 32;
  const int rg = (t.row0 + g.wr) / 32;
  float* gb_m = gb_part + ((long)m * nrg + rg) * n;

  // the walk of epi_cols/epi_rows, written out (see above)
#pragma unroll
  for (int tj = 0; tj < NACC; ++tj) {
#pragma clang fp contract(off)
    int col = t.col0 + g.wc + tj * 32 + g.l31;
    bool col_ok = ALIGNED || col < n;
    float colsum = 0.f;
#pragma unroll
    for (int r_ = 0; r_ < 16; ++r_) {
      int row = t.row0 + g.wr + acc_row(r_, g.lane);
      if ((ALIGNED || row < B) && col_ok) {
        float cv = ei.ref(c_m, row, col, r_, tj);
        float gv;
        if (gc_mode == GC_REVERSE) {
          // reverse SAE: active set is cv != 0, l1 grad is sign(cv), and
          // the bias receives no gradient from the code path
          float sgn = (cv > 0.f) ? 1.f : ((cv < 0.f) ? -1.f : 0.f);
          gv = (cv != 0.f) ? (gscale * t.acc[tj][r_] + l1_term * sgn) : 0.f;
        } else {
          gv = (cv > 0.f) ? fmaf(gscale, t.acc[tj][r_], l1_term) : 0.f;
        }
        ei.ref(g_m, row, col, r_, tj) = gv;
        colsum += gv;
      }
    }
    float tot;
    if (col_ok && gc_mode == GC_RELU && halfwave_pair_sum(g, colsum, tot) && (ALIGNED || rg < nrg))
      gb_m[col] = tot;
  }
}

// g_bias[m, col] (+)= sum over the nrg row groups of part[m, rg, col], in a
// fixed order: 64 columns per block, the groups split into 4 contiguous slices
// (one wave each, summed ascending), the 4 slice sums combined pairwise.
extern "C" __global__ __launch_bounds__(256)
void k_colsum_groups(const float* __restrict__ part,  // [M, nrg, n]
                     float* __restrict__ g_bias,      // [M, n]
                     int nrg, int n, long total,      // total = M * n
                     int accumulate) {
  __shared__ float sh[4][WAVE];
  const int lc = threadIdx.x & (WAVE - 1);
  const int sl = threadIdx.x / WAVE;
  const long i = (long)blockIdx.x * WAVE + lc;
  float s = 0.f;
  if (i < total) {
    const long m = i / n;
    const int col = (int)(i - m * n);
    const float* p = part + m * nrg * n + col;
    const int per = (nrg + 3) / 4;
    const int lo = sl * per;
    const int hi = min(nrg, lo + per);
#pragma unroll 16
    for (int rg = lo; rg < hi; ++rg) s += p[(long)rg * n];
  }
  sh[sl][lc] = s;
  __syncthreads();
  if (sl == 0 && i < total) {
    float t = (sh[0][lc] + sh[1][lc]) + (sh[2][lc] + sh[3][lc]);
    g_bias[i] = accumulate ? g_bias[i] + t : t;
  }
}

// ---------------------------------------------------------------------------
// k_gc_thresh_t: backward of the thresholding SAE's gate (K15).
// Same GEMM as k_gc_t (acc = r @ What^T); epilogue turns dL/dcode into
//   gpre   = dL/dc      = gv * g'(u) * a^2/max(a^2,eps)   (feeds grad_w)
//   g_gain = sum_b dL/dgain = same weight as gpre (column sum)
//   g_scale= sum_b dL/da = gv * 2a * (g(u) - [a^2>eps] g'(u) u a^2/max(..))
// with gv = gscale*acc + l1/B * [code>0].
// ---------------------------------------------------------------------------
template <int TBK, int MINW, int TBN = BN, bool ALIGNED = false>
__global__ __launch_bounds__(NTHREADS, MINW)
void k_gc_thresh_t(const float* r,                     // [M, B, d]  (staged operands: no
                   const float* Wdec,                  // [M, n, d]   __restrict__, see gemm_mainloop)
                   const float* __restrict__ inv_norms,// [M, n]
                   const float* __restrict__ c,        // [M, B, n] (codes)
                   const float* __restrict__ u,        // [M, B, n]
                   const float* __restrict__ act_scale,// [M, n]
                   const float* __restrict__ l1_alpha, // [M]
                   float* __restrict__ gpre_out,       // [M, B, n]
                   float* __restrict__ g_gain,         // [M, n]
                   float* __restrict__ g_scale,        // [M, n]
                   int B, int d, int n, int prio) {
  __shared__ TLds<TBK, BM> As;
  __shared__ TLds<TBK, TBN> Bs;

  constexpr int NACC = Tile<TBN>::NACC;
  Tile<TBN> t(prio);
  const int m = t.m;
  const float* r_m = r + (long)m * B * d;
  const float* W = Wdec + (long)m * n * d;
  const float* inv = inv_norms + (long)m * n;
  const float* c_m = c + (long)m * B * n;
  const float* u_m = u + (long)m * B * n;
  const float gscale = 2.0f / ((float)B * (float)d);
  const float l1_term = l1_alpha[m] / (float)B;

  TStage<TBK, BM> sa;
  TStage<TBK, TBN> sb;
  stage_T_scale<TBK, TBN, ALIGNED>(inv, t.col0, n, sb);
  gemm_mainloop<TBK>(
      d, As, Bs, t.acc,
      [&](int k0) { stage_T_load<TBK, BM, ALIGNED>(r_m, d, t.row0, k0, B, d, sa); },
      [&](int k0) { stage_T_load<TBK, TBN, ALIGNED>(W, d, t.col0, k0, n, d, sb); },
      [&](int buf) { stage_T_write(sa, As, buf, false); },
      [&](int buf) { stage_T_write(sb, Bs, buf, true); });

  const EpiGeom g = epi_geom<NACC>();
  EpiIndex<ALIGNED> ei(t.row0, t.col0, n, g);
  float* g_m = gpre_out + (long)m * B * n;
  float* gg_m = g_gain + (long)m * n;
  float* gs_m = g_scale + (long)m * n;

  // The traversal is written out here for the same reason as in k_gc_t: with
  // epi_cols/epi_rows the aligned <16, 8, 128> variant went from 63 to 64
  // VGPRs and measured about 1% slower (profiles/README.md, r04).
#pragma unroll
  for (int tj = 0; tj < NACC; ++tj) {
#pragma clang fp contract(off)
    int col = t.col0 + g.wc + tj * 32 + g.l31;
    bool col_ok = ALIGNED || col < n;
    float a = col_ok ? act_scale[(long)m * n + col] : 1.f;
    float s_raw = a * a;
    float s = fmaxf(s_raw, GATE_EPS);
    float clamp_act = (s_raw > GATE_EPS) ? 1.f : 0.f;  // clamp passes grad?
    float f = s_raw / s;  // a^2 / clamp(a^2): ==1 away from the clamp
    float gain_colsum = 0.f, scale_colsum = 0.f;
#pragma unroll
    for (int r_ = 0; r_ < 16; ++r_) {
      int row = t.row0 + g.wr + acc_row(r_, g.lane);
      if ((ALIGNED || row < B) && col_ok) {
        auto at = [&](auto* p) -> auto& { return ei.ref(p, row, col, r_, tj); };
        float code = at(c_m);
        float uv = at(u_m);
        float gp = gate_gp(uv);
        float gv = fmaf(gscale, t.acc[tj][r_], (code > 0.f) ? l1_term : 0.f);
        float gc_ = gv * gp * f;
        at(g_m) = gc_;
        gain_colsum += gc_;
        scale_colsum += gv * 2.0f * a * (gate_g(uv) - clamp_act * gp * uv * f);
      }
    }
    if (col_ok) {
      float gain_tot, scale_tot;
      const bool owner = halfwave_pair_sum(g, gain_colsum, gain_tot);
      halfwave_pair_sum(g, scale_colsum, scale_tot);
      if (owner) {
        if (gain_tot != 0.f) atomicAdd(&gg_m[col], gain_tot);
        if (scale_tot != 0.f) atomicAdd(&gs_m[col], scale_tot);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// k_lista_bwd_elem: one pass over [M, B, n] replacing the LISTA backward's
// elementwise chain:
//   g_x   = (1 + m) g_y + carry_in
//   g_r   = g_x * [|r| > theta]
//   carry = -m g_y                       (becomes next layer's carry_in)
//   g_theta[col] += -g_r * sign(r)       (column sum)
//   g_rho[model] += g_y * (x - x_prev)   (scalar sum; clamp gate on host)
// grid (ceil(n/256), ceil(B/ROWS), M); block 256; coalesced row-major loops.
// ---------------------------------------------------------------------------
#define LBW_COLS 256
#define LBW_ROWS 256
extern "C" __global__ __launch_bounds__(LBW_COLS)
void k_lista_bwd_elem(const float* __restrict__ g_y,
                      const float* __restrict__ carry_in,  // nullptr on layer L
                      const float* __restrict__ r,
                      const float* __restrict__ theta,   // [M, n]
                      const float* __restrict__ x,
                      const float* __restrict__ x_prev,
                      const float* __restrict__ mom,     // [M]
                      float* __restrict__ g_r,
                      float* __restrict__ carry_out,
                      float* __restrict__ g_theta,       // [M, n] (pre-zeroed)
                      float* __restrict__ g_rho,         // [M]    (pre-zeroed)
                      int B, int n) {
  const int m = blockIdx.z;
  const int col = blockIdx.x * LBW_COLS + threadIdx.x;
  const int row0 = blockIdx.y * LBW_ROWS;
  const int row1 = min(row0 + LBW_ROWS, B);
  const bool col_ok = col < n;
  const float mm = mom[m];
  const float th = col_ok ? theta[(long)m * n + col] : 0.f;
  const long base = (long)m * B * n;

  float th_sum = 0.f, rho_sum = 0.f;
  if (col_ok) {
    for (int row = row0; row < row1; ++row) {
      long idx = base + (long)row * n + col;
      float gy = g_y[idx];
      float gx = (1.0f + mm) * gy + (carry_in ? carry_in[idx] : 0.f);
      float rv = r[idx];
      float gr = (fabsf(rv) > th) ? gx : 0.f;
      g_r[idx] = gr;
      carry_out[idx] = -mm * gy;
      th_sum -= gr * ((rv > 0.f) ? 1.f : ((rv < 0.f) ? -1.f : 0.f));
      rho_sum += gy * (x[idx] - x_prev[idx]);
    }
    if (th_sum != 0.f) atomicAdd(&g_theta[(long)m * n + col], th_sum);
  }
  rho_sum = wave_reduce_sum(rho_sum);
  __shared__ float warp_part[LBW_COLS / WAVE];
  if ((threadIdx.x & (WAVE - 1)) == 0) warp_part[threadIdx.x / WAVE] = rho_sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f;
    for (int w = 0; w < LBW_COLS / WAVE; ++w) s += warp_part[w];
    if (s != 0.f) atomicAdd(&g_rho[m], s);
  }
}

// ---------------------------------------------------------------------------
// k_topk_select: per-row top-k selection + scatter for the TopK encoder
// (SURVEY.md K8).  One 256-thread block per (model, batch-row); exact
// radix select over the order-preserving uint mapping of fp32 (4 passes of
// 8-bit histograms), then one write pass producing the dense code row
//   c[j] = j in top-k ? max(score[j], 0) : 0     (reference topk_encoder.py
// keeps clamped values in the selected slots), with fired counts fused.
// Exact-equal ties at the threshold are admitted in arbitrary order via an
// LDS slot counter (measure-zero for continuous scores).
// ---------------------------------------------------------------------------
#define TOPK_T 256
__device__ __forceinline__ unsigned f32_ord(float f) {
  unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

extern "C" __global__ __launch_bounds__(TOPK_T)
void k_topk_select(const float* __restrict__ scores,  // [M, B, n]
                   float* __restrict__ c_out,         // [M, B, n]
                   float* __restrict__ fired,         // [M, n]
                   const int* __restrict__ ks,        // [M]
                   int B, int n) {
  const int m = blockIdx.z;
  const int row = blockIdx.x;
  if (row >= B) return;
  const float* s = scores + ((long)m * B + row) * n;
  float* c = c_out + ((long)m * B + row) * n;
  float* fired_m = fired + (long)m * n;
  int k = ks[m];
  if (k >= n) k = n;

  __shared__ unsigned hist[256];
  __shared__ unsigned sh_prefix, sh_mask, sh_kleft, sh_slots;

  if (threadIdx.x == 0) {
    sh_prefix = 0u;
    sh_mask = 0u;  // bits of the prefix that are decided
    sh_kleft = (unsigned)k;
  }
  __syncthreads();

  // 4 radix passes, MSB first
  for (int shift = 24; shift >= 0; shift -= 8) {
    if (threadIdx.x < 256) hist[threadIdx.x] = 0u;
    __syncthreads();
    unsigned prefix = sh_prefix, mask = sh_mask;
    for (int j = threadIdx.x; j < n; j += TOPK_T) {
      unsigned u = f32_ord(s[j]);
      if ((u & mask) == prefix) atomicAdd(&hist[(u >> shift) & 0xFFu], 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned kleft = sh_kleft;
      int bin = 255;
      for (; bin >= 0; --bin) {
        if (hist[bin] >= kleft) break;
        kleft -= hist[bin];
      }
      if (bin < 0) bin = 0;  // defensive; cannot happen for k <= n
      sh_kleft = kleft;
      sh_prefix = sh_prefix | ((unsigned)bin << shift);
      sh_mask = sh_mask | (0xFFu << shift);
    }
    __syncthreads();
  }

  // threshold = exact k-th largest key; elements with key > thr are all
  // selected; sh_kleft of the == thr ties are selected in index order
  unsigned thr = sh_prefix;
  if (threadIdx.x == 0) sh_slots = sh_kleft;
  __syncthreads();
  for (int j = threadIdx.x; j < n; j += TOPK_T) {
    unsigned u = f32_ord(s[j]);
    float v = 0.f;
    bool sel = u > thr;
    if (!sel && u == thr) {
      unsigned slot = atomicSub(&sh_slots, 1u);
      sel = (slot != 0u && slot <= (unsigned)n);  // old value; wraps reject
    }
    if (sel) {
      v = fmaxf(s[j], 0.f);
      if (v > 0.f) atomicAdd(&fired_m[j], 1.f);
    }
    c[j] = v;
  }
}

// ---------------------------------------------------------------------------
// k_btk_hist / k_btk_write: batch-level top-k selection for the BatchTopK
// encoder.  Per model, the K = min(k*B, B*n) largest of ALL B*n scores are
// kept (not k per row): t = the K-th largest score of the whole matrix,
//   c[b,j] = (s[b,j] >= t && s[b,j] > 0) ? s[b,j] : +0
// with every exact tie at t kept, so the result does not depend on any order.
//
// B*n is millions of scores per model, so the exact radix select over the
// f32_ord keys runs across many workgroups per model (blockIdx.z = model),
// split over kernel launches on one stream; no workgroup ever waits for
// another.  Three histogram passes, MSB first, 11 + 11 + 10 bits:
//   k_btk_hist<P>: every block counts its grid-stride slice of the scores
//     whose key matches the prefix decided so far into an LDS histogram
//     (BTK_R lane-interleaved copies per bin: scores cluster in a few
//     exponent buckets, and lanes of one wave that hit the same bin would
//     serialise on one LDS address), then adds its non-empty bins to the
//     model's global histogram of that pass: integer atomics, one per bin
//     and block.
//   The bin holding the K-th element of pass P is picked at the head of the
//     next launch, by every block redundantly (btk_pick, a block-wide scan
//     from the top bin down); block 0 records (prefix, rank left) in the
//     workspace for the launch after that, so each launch picks once.
//   k_btk_write: picks the last bin -> the exact key of t; one pass writes c
//     and the fired counts; block 0 reports t and folds max(t, 0) into the
//     running inference threshold.
// Scores are read as float4 where the model's base pointer allows it, with a
// scalar tail (and a scalar loop otherwise): the counts are the same.
//
// Workspace, int32, BTK_WORK per model, zeroed by the launcher before the
// first pass: hist0[2048] hist1[2048] hist2[1024] state[BTK_STATE].
// ---------------------------------------------------------------------------
#define BTK_T 256
#define BTK_R 4
#define BTK_BINS0 2048
#define BTK_BINS1 2048
#define BTK_BINS2 1024
#define BTK_HIST1 BTK_BINS0
#define BTK_HIST2 (BTK_BINS0 + BTK_BINS1)
#define BTK_STATE_OFF (BTK_BINS0 + BTK_BINS1 + BTK_BINS2)
#define BTK_STATE 8  // (prefix, rank left) after pass 0 and after pass 1
#define BTK_WORK (BTK_STATE_OFF + BTK_STATE)

__device__ __forceinline__ float f32_unord(unsigned u) {
  return __uint_as_float((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u);
}

// K of one model: min(k * B, B * n), 0 for k <= 0
__device__ __forceinline__ long btk_K(int k, int B, long Nm) {
  if (k <= 0) return 0;
  long K = (long)k * B;
  return K < Nm ? K : Nm;
}

// The bin of the global histogram gh[nbins] that holds the kleft-th largest
// counted element, scanning from the top bin down: out[0] = bin, out[1] =
// its rank inside that bin.  Whole block, nbins = BTK_T * PER.
template <int PER>
__device__ __forceinline__ void btk_pick(const unsigned* __restrict__ gh, unsigned kleft,
                                         unsigned* sh_scan, unsigned* out) {
  const int t = threadIdx.x;
  const int top = BTK_T * PER - 1 - t * PER;  // this thread's highest bin
  unsigned cnt[PER];
  unsigned part = 0u;
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    cnt[i] = gh[top - i];
    part += cnt[i];
  }
  if (t == 0) {  // defensive: the counts always reach kleft
    out[0] = 0u;
    out[1] = kleft;
  }
  unsigned v = part;  // inclusive count from the top bin through this thread's
  for (int off = 1; off < BTK_T; off <<= 1) {
    sh_scan[t] = v;
    __syncthreads();
    if (t >= off) v += sh_scan[t - off];
    __syncthreads();
  }
  const unsigned excl = v - part;
  if (excl < kleft && kleft <= v) {  // one thread
    unsigned left = kleft - excl;
    int i = 0;
    for (; i < PER - 1; ++i) {
      if (cnt[i] >= left) break;
      left -= cnt[i];
    }
    out[0] = (unsigned)(top - i);
    out[1] = left;
  }
  __syncthreads();
}

template <int SHIFT, int NBINS>
__device__ __forceinline__ void btk_count(unsigned* hist, float s, unsigned mask,
                                          unsigned prefix, int rep) {
  unsigned u = f32_ord(s);
  if ((u & mask) == prefix) atomicAdd(&hist[((u >> SHIFT) & (NBINS - 1)) * BTK_R + rep], 1u);
}

template <int PASS>
__global__ __launch_bounds__(BTK_T)
void k_btk_hist(const float* __restrict__ scores,  // [M, B, n]
                const int* __restrict__ ks,        // [M]
                unsigned* __restrict__ work,       // [M, BTK_WORK]
                int B, int n) {
  constexpr int SHIFT = PASS == 0 ? 21 : (PASS == 1 ? 10 : 0);
  constexpr int NBINS = PASS == 0 ? BTK_BINS0 : (PASS == 1 ? BTK_BINS1 : BTK_BINS2);
  constexpr int HOFF = PASS == 0 ? 0 : (PASS == 1 ? BTK_HIST1 : BTK_HIST2);
  constexpr unsigned MASK = PASS == 0 ? 0u : (PASS == 1 ? 0xFFE00000u : 0xFFFFFC00u);

  const int m = blockIdx.z;
  const int t = threadIdx.x;
  const long Nm = (long)B * n;
  const long K = btk_K(ks[m], B, Nm);
  if (K == 0) return;  // whole block: nothing is selected
  unsigned* work_m = work + (long)m * BTK_WORK;

  __shared__ __attribute__((aligned(16))) unsigned hist[NBINS * BTK_R];
  __shared__ unsigned sh_scan[BTK_T];
  __shared__ unsigned sh_pick[2];

  for (int i = t; i < NBINS * BTK_R; i += BTK_T) hist[i] = 0u;

  unsigned prefix = 0u;
  if (PASS == 1) {
    btk_pick<BTK_BINS0 / BTK_T>(work_m, (unsigned)K, sh_scan, sh_pick);
    prefix = sh_pick[0] << 21;
    if (blockIdx.x == 0 && t == 0) {
      work_m[BTK_STATE_OFF + 0] = prefix;
      work_m[BTK_STATE_OFF + 1] = sh_pick[1];
    }
  } else if (PASS == 2) {
    prefix = work_m[BTK_STATE_OFF + 0];
    btk_pick<BTK_BINS1 / BTK_T>(work_m + BTK_HIST1, work_m[BTK_STATE_OFF + 1], sh_scan, sh_pick);
    prefix |= sh_pick[0] << 10;
    if (blockIdx.x == 0 && t == 0) {
      work_m[BTK_STATE_OFF + 2] = prefix;
      work_m[BTK_STATE_OFF + 3] = sh_pick[1];
    }
  }
  __syncthreads();  // hist zeroed (the picks end on a barrier as well)

  const float* s = scores + (long)m * Nm;
  const int rep = t & (BTK_R - 1);
  const long stride = (long)gridDim.x * BTK_T;
  const long first = (long)blockIdx.x * BTK_T + t;
  const bool vec = (reinterpret_cast<uintptr_t>(s) & 15) == 0;
  const long nvec = vec ? (Nm >> 2) : 0;
  const float4* s4 = reinterpret_cast<const float4*>(s);
  long i = first;
  for (; i + 3 * stride < nvec; i += 4 * stride) {  // four loads in flight
    float4 v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = s4[i + q * stride];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      btk_count<SHIFT, NBINS>(hist, v[q].x, MASK, prefix, rep);
      btk_count<SHIFT, NBINS>(hist, v[q].y, MASK, prefix, rep);
      btk_count<SHIFT, NBINS>(hist, v[q].z, MASK, prefix, rep);
      btk_count<SHIFT, NBINS>(hist, v[q].w, MASK, prefix, rep);
    }
  }
  for (; i < nvec; i += stride) {
    float4 v = s4[i];
    btk_count<SHIFT, NBINS>(hist, v.x, MASK, prefix, rep);
    btk_count<SHIFT, NBINS>(hist, v.y, MASK, prefix, rep);
    btk_count<SHIFT, NBINS>(hist, v.z, MASK, prefix, rep);
    btk_count<SHIFT, NBINS>(hist, v.w, MASK, prefix, rep);
  }
  for (long j = (nvec << 2) + first; j < Nm; j += stride)
    btk_count<SHIFT, NBINS>(hist, s[j], MASK, prefix, rep);
  __syncthreads();

  unsigned* gh = work_m + HOFF;
  const uint4* hist4 = reinterpret_cast<const uint4*>(hist);  // BTK_R == 4 copies
  for (int bin = t; bin < NBINS; bin += BTK_T) {
    uint4 h = hist4[bin];
    unsigned c = h.x + h.y + h.z + h.w;
    if (c) atomicAdd(&gh[bin], c);
  }
}

__device__ __forceinline__ float btk_keep(float s, unsigned thr, float* __restrict__ fired_m,
                                          long idx, int n) {
  if (f32_ord(s) >= thr && s > 0.f) {
    atomicAdd(&fired_m[idx % n], 1.f);  // whole numbers: exact in any order
    return s;
  }
  return 0.f;
}

__global__ __launch_bounds__(BTK_T)
void k_btk_write(const float* __restrict__ scores,  // [M, B, n]
                 float* __restrict__ c_out,         // [M, B, n]
                 float* __restrict__ fired,         // [M, n]
                 const int* __restrict__ ks,        // [M]
                 float* __restrict__ thr_out,       // [M]
                 const unsigned* __restrict__ work, // [M, BTK_WORK]
                 float* __restrict__ theta,         // [M] or null
                 int* __restrict__ theta_n,         // [M] or null
                 const float* __restrict__ theta_lr,  // [M] or null
                 int B, int n) {
  const int m = blockIdx.z;
  const int t = threadIdx.x;
  const long Nm = (long)B * n;
  const long K = btk_K(ks[m], B, Nm);
  const unsigned* work_m = work + (long)m * BTK_WORK;

  __shared__ unsigned sh_scan[BTK_T];
  __shared__ unsigned sh_pick[2];

  // K == 0 keeps nothing: no key reaches 0xFFFFFFFF with s > 0 (that is a NaN)
  unsigned thr = 0xFFFFFFFFu;
  if (K != 0) {
    btk_pick<BTK_BINS2 / BTK_T>(work_m + BTK_HIST2, work_m[BTK_STATE_OFF + 3], sh_scan, sh_pick);
    thr = work_m[BTK_STATE_OFF + 2] | sh_pick[0];
  }

  if (blockIdx.x == 0 && t == 0) {
    const float tval = K != 0 ? f32_unord(thr) : __uint_as_float(0x7F800000u);
    thr_out[m] = tval;
    if (theta != nullptr && K != 0) {
      const float stat = fmaxf(tval, 0.f);
      const int cnt = theta_n[m];
      float th = theta[m];
      if (cnt == 0) th = stat;
      else if (stat != th) th = fmaf(theta_lr[m], stat - th, th);  // two roundings
      theta[m] = th;
      theta_n[m] = cnt + 1;
    }
  }

  const float* s = scores + (long)m * Nm;
  float* c = c_out + (long)m * Nm;
  float* fired_m = fired + (long)m * n;
  const long stride = (long)gridDim.x * BTK_T;
  const long first = (long)blockIdx.x * BTK_T + t;
  const bool vec = ((reinterpret_cast<uintptr_t>(s) | reinterpret_cast<uintptr_t>(c)) & 15) == 0;
  const long nvec = vec ? (Nm >> 2) : 0;
  const float4* s4 = reinterpret_cast<const float4*>(s);
  float4* c4 = reinterpret_cast<float4*>(c);
  for (long i = first; i < nvec; i += stride) {
    float4 v = s4[i];
    float4 o;
    o.x = btk_keep(v.x, thr, fired_m, 4 * i + 0, n);
    o.y = btk_keep(v.y, thr, fired_m, 4 * i + 1, n);
    o.z = btk_keep(v.z, thr, fired_m, 4 * i + 2, n);
    o.w = btk_keep(v.w, thr, fired_m, 4 * i + 3, n);
    c4[i] = o;
  }
  for (long j = (nvec << 2) + first; j < Nm; j += stride)
    c[j] = btk_keep(s[j], thr, fired_m, j, n);
}

// ---------------------------------------------------------------------------
// k_grad_w_t
// ---------------------------------------------------------------------------
template <int TBK, int MINW, int TBN = BN, bool ALIGNED = false>
__global__ __launch_bounds__(NTHREADS, MINW)
void k_grad_w_t(const float* P, long p_batch_stride,  // staged operands: no __restrict__,
                const float* Q, long q_batch_stride,  // see gemm_mainloop
                float* __restrict__ gw,  // [M, n, d]
                float alpha, float beta,
                int B, int n, int d, int prio) {
  __shared__ DLds<TBK, BM> As;
  __shared__ DLds<TBK, TBN> Bs;

  constexpr int NACC = Tile<TBN>::NACC;
  Tile<TBN> t(prio);  // row0: n rows, col0: d cols
  const int m = t.m;
  const float* P_m = P + (long)m * p_batch_stride;
  const float* Q_m = Q + (long)m * q_batch_stride;

  DStage<TBK, BM> sa;
  DStage<TBK, TBN> sb;
  gemm_mainloop<TBK>(
      B, As, Bs, t.acc,
      [&](int k0) { stage_D_load<TBK, BM, ALIGNED>(P_m, n, k0, t.row0, B, n, nullptr, sa); },
      [&](int k0) { stage_D_load<TBK, TBN, ALIGNED>(Q_m, d, k0, t.col0, B, d, nullptr, sb); },
      [&](int buf) { stage_D_write(sa, As, buf, false); },
      [&](int buf) { stage_D_write(sb, Bs, buf, false); });

  const EpiGeom g = epi_geom<NACC>();
  EpiIndex<ALIGNED> ei(t.row0, t.col0, d, g);
  float* gw_m = gw + (long)m * n * d;

  epi_cols<NACC, ALIGNED>(g, t.col0, d, [&](int tj, int col, bool col_ok) {
#pragma clang fp contract(off)
    epi_rows<ALIGNED>(g, ei, t.row0, n, tj, col, col_ok, [&](int r, auto at) {
      float v = alpha * t.acc[tj][r];
      if (beta != 0.f) v = fmaf(beta, at(gw_m), v);
      at(gw_m) = v;
    });
  });
}

// ---------------------------------------------------------------------------
// k_project_adam: per dictionary row i of model m:
//   if project: g = (gw - (gw . w)/norm^2 * w * [norm>eps]) / max(norm,eps)
//   Adam with per-model bias correction.
// One wave per row; 8 rows per block.
// ---------------------------------------------------------------------------
extern "C" __global__ __launch_bounds__(NTHREADS)
void k_project_adam(float* __restrict__ W,        // [M*n, d]
                    const float* __restrict__ gw, // [M*n, d]
                    const float* __restrict__ norms,  // [M*n]
                    float* __restrict__ mu, float* __restrict__ nu,
                    const float* __restrict__ step_no,  // [M]
                    int n_rows_total, int n_per_model, int d,
                    float lr, float b1, float b2, float eps_adam,
                    float eps_norm, int project,
                    const float* __restrict__ w_used_p,  // nullptr -> W
                    int clamp_mask,  // 1: g *= [W >= 0] (clamp backward)
                    const float* __restrict__ lr_mult) { // [M*n] per-row lr
                                                         // scale (post-resample
                                                         // warmup) or nullptr
  const int wave = threadIdx.x / WAVE;
  const int lane = threadIdx.x & (WAVE - 1);
  const int row = blockIdx.x * (NTHREADS / WAVE) + wave;
  if (row >= n_rows_total) return;
  const float lr_eff = lr_mult ? lr * lr_mult[row] : lr;

  float* w_param = W + (long)row * d;
  const float* w = w_used_p ? w_used_p + (long)row * d : w_param;
  const float* g_in = gw + (long)row * d;
  float* mu_r = mu + (long)row * d;
  float* nu_r = nu + (long)row * d;

  const int m = row / n_per_model;
  const float t = step_no[m];
  const float bc1 = 1.0f - powf(b1, t);
  const float bc2 = 1.0f - powf(b2, t);

  float inv_s = 1.0f, dot_scaled = 0.f;
  bool do_proj = false;
  if (project) {
    float nrm = norms[row];
    float s = fmaxf(nrm, eps_norm);
    inv_s = 1.0f / s;
    do_proj = nrm > eps_norm;
    if (do_proj) {
      float acc = 0.f;
      for (int j = lane; j < d; j += WAVE) acc += g_in[j] * w[j];
      acc = wave_reduce_sum(acc);
      dot_scaled = acc / (nrm * nrm);
    }
  }

  for (int j = lane; j < d; j += WAVE) {
    float g = g_in[j];
    if (project) {
      if (do_proj) g = (g - dot_scaled * w[j]) * inv_s;
      else g = g * inv_s;
    }
    if (clamp_mask && w_param[j] < 0.f) g = 0.f;
    float m1 = b1 * mu_r[j] + (1.0f - b1) * g;
    float v1 = b2 * nu_r[j] + (1.0f - b2) * g * g;
    mu_r[j] = m1;
    nu_r[j] = v1;
    w_param[j] -= lr_eff * (m1 / bc1) / (sqrtf(v1 / bc2) + eps_adam);
  }
}

// ---------------------------------------------------------------------------
// k_bias_adam: Adam on [M, n] bias with optional L2-norm decay gradient.
// grid (M); block NTHREADS.
// ---------------------------------------------------------------------------
extern "C" __global__ __launch_bounds__(NTHREADS)
void k_bias_adam(float* __restrict__ bias,        // [M, n]
                 const float* __restrict__ g_bias,// [M, n]
                 const float* __restrict__ bias_decay, // [M]
                 float* __restrict__ mu, float* __restrict__ nu,
                 const float* __restrict__ step_no,
                 int n, float lr, float b1, float b2, float eps_adam,
                 const float* __restrict__ lr_mult) { // [M, n] or nullptr
  const int m = blockIdx.x;
  const float* lrm_m = lr_mult ? lr_mult + (long)m * n : nullptr;
  float* b_m = bias + (long)m * n;
  const float* g_m = g_bias + (long)m * n;
  float* mu_m = mu + (long)m * n;
  float* nu_m = nu + (long)m * n;
  const float bd = bias_decay[m];
  const float t = step_no[m];
  const float bc1 = 1.0f - powf(b1, t);
  const float bc2 = 1.0f - powf(b2, t);

  __shared__ float partial[NTHREADS / WAVE];
  __shared__ float norm_sq_s;
  float decay_scale = 0.f;
  if (bd != 0.f) {
    float acc = 0.f;
    for (int j = threadIdx.x; j < n; j += NTHREADS) acc += b_m[j] * b_m[j];
    acc = wave_reduce_sum(acc);
    if ((threadIdx.x & (WAVE - 1)) == 0) partial[threadIdx.x / WAVE] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
      float s = 0.f;
      for (int wv = 0; wv < NTHREADS / WAVE; ++wv) s += partial[wv];
      norm_sq_s = s;
    }
    __syncthreads();
    float nrm = sqrtf(norm_sq_s);
    decay_scale = (nrm > 0.f) ? bd / nrm : 0.f;
  }

  for (int j = threadIdx.x; j < n; j += NTHREADS) {
    float g = g_m[j] + decay_scale * b_m[j];
    float m1 = b1 * mu_m[j] + (1.0f - b1) * g;
    float v1 = b2 * nu_m[j] + (1.0f - b2) * g * g;
    mu_m[j] = m1;
    nu_m[j] = v1;
    float lr_eff = lrm_m ? lr * lrm_m[j] : lr;
    b_m[j] -= lr_eff * (m1 / bc1) / (sqrtf(v1 / bc2) + eps_adam);
  }
}

// ---------------------------------------------------------------------------
// k_resample: the dead-neuron resampling rule fully fused:
// one block per model scans the fired counters, ranks dead features in
// index order (block-wide ballot prefix over 256-column segments), and for
// the first n_track of them overwrites the encoder row with the matching
// worst-example direction (scaled), zeroes the Adam moments, resets the
// bias (+its moments), and optionally rewrites a decoder row.  No host loop,
// no per-model syncs; counts land in counts_out.
// ---------------------------------------------------------------------------
#define RSMP_T 256
extern "C" __global__ __launch_bounds__(RSMP_T)
void k_resample(const float* __restrict__ fired,      // [M, n]
                const float* __restrict__ new_rows,   // [M, T, d] unit dirs
                const float* __restrict__ enc_scale,  // [M] row-norm scale
                float* __restrict__ W,                // [M, n, d] encoder
                float* __restrict__ mu_w, float* __restrict__ nu_w,
                float* __restrict__ dec,              // [M, n, d] or nullptr
                float* __restrict__ mu_d, float* __restrict__ nu_d,
                float* __restrict__ bias,             // [M, n] or nullptr
                float* __restrict__ mu_b, float* __restrict__ nu_b,
                int* __restrict__ counts_out,         // [M]
                int n, int d, int n_track) {
  const int m = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wave = tid / WAVE;
  const float* fired_m = fired + (long)m * n;
  const float scale = enc_scale[m];

  __shared__ int base;
  __shared__ int wave_cnt[RSMP_T / WAVE];
  if (tid == 0) base = 0;
  __syncthreads();

  for (int s0 = 0; s0 < n; s0 += RSMP_T) {
    int j = s0 + tid;
    bool isdead = (j < n) && (fired_m[j] == 0.0f);
    unsigned long long mask = __ballot(isdead);
    int lane_rank = __popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) wave_cnt[wave] = __popcll(mask);
    __syncthreads();
    int wave_prefix = 0;
    for (int w = 0; w < wave; ++w) wave_prefix += wave_cnt[w];
    int rank = base + wave_prefix + lane_rank;
    if (isdead && rank < n_track) {
      const float* src = new_rows + ((long)m * n_track + rank) * d;
      float* w_row = W + ((long)m * n + j) * d;
      float* muw = mu_w + ((long)m * n + j) * d;
      float* nuw = nu_w + ((long)m * n + j) * d;
      for (int t = 0; t < d; ++t) {
        float v = src[t];
        w_row[t] = v * scale;
        muw[t] = 0.f;
        nuw[t] = 0.f;
      }
      if (dec) {
        float* d_row = dec + ((long)m * n + j) * d;
        float* mud = mu_d + ((long)m * n + j) * d;
        float* nud = nu_d + ((long)m * n + j) * d;
        for (int t = 0; t < d; ++t) {
          d_row[t] = src[t];
          mud[t] = 0.f;
          nud[t] = 0.f;
        }
      }
      if (bias) {
        bias[(long)m * n + j] = 0.f;
        mu_b[(long)m * n + j] = 0.f;
        nu_b[(long)m * n + j] = 0.f;
      }
    }
    __syncthreads();
    if (tid == 0) {
      int tot = 0;
      for (int w = 0; w < RSMP_T / WAVE; ++w) tot += wave_cnt[w];
      base += tot;
    }
    __syncthreads();
    if (base >= n_track && s0 + RSMP_T < n) {
      // everything past here would exceed the replacement budget; still
      // need the total dead count? reference reports replaced count only.
      break;
    }
  }
  if (tid == 0) counts_out[m] = base < n_track ? base : n_track;
}

// ---------------------------------------------------------------------------
// k_colsum: out[m, j] = alpha * sum_b X[m, b, j] for X [M, B, n].
// The column-sum tail of the residual/semilinear backward: torch's strided
// reduce runs this at ~140 GB/s (profiles/r02_*_kernel_stats.csv); here each
// 256-thread block owns 256 consecutive columns of one (model, B-slice) so
// every row read is one fully-coalesced 1 KB line burst, and the B axis is
// split over grid.z (partials combined with atomicAdd; caller zero-fills
// out) to keep >= 4k waves in flight on the 256-CU chip.
#define COLSUM_T 256
extern "C" __global__ __launch_bounds__(COLSUM_T)
void k_colsum(const float* __restrict__ X, float* __restrict__ out,
              int B, int n, float alpha, int absval) {
  const int j = blockIdx.x * COLSUM_T + threadIdx.x;
  const int m = blockIdx.y;
  const int nsplit = gridDim.z;
  if (j >= n) return;
  const long base = (long)m * B * n;
  const int b0 = (int)(((long)blockIdx.z * B) / nsplit);
  const int b1 = (int)(((long)(blockIdx.z + 1) * B) / nsplit);
  float acc = 0.f;
  if (absval) {
    #pragma unroll 4
    for (int b = b0; b < b1; ++b) acc += fabsf(X[base + (long)b * n + j]);
  } else {
    #pragma unroll 4
    for (int b = b0; b < b1; ++b) acc += X[base + (long)b * n + j];
  }
  atomicAdd(&out[(long)m * n + j], acc * alpha);
}

// ---------------------------------------------------------------------------
// k_transpose_scale: dst[c][r] = src[r][c] * (scale ? scale[r] : 1), batched
// over grid.z with explicit strides.  64x64 LDS tiles, coalesced both sides.
// Feeds the all-direct-staged GEMM variants below (x^T, r^T, What^T).
// ---------------------------------------------------------------------------
extern "C" __global__ __launch_bounds__(256)
void k_transpose_scale(const float* __restrict__ src, float* __restrict__ dst,
                       const float* __restrict__ scale,
                       int R, int C,
                       long src_mstride, long dst_mstride, long scale_mstride) {
  __shared__ float tile[64][65];
  const int m = blockIdx.z;
  src += (long)m * src_mstride;
  dst += (long)m * dst_mstride;
  if (scale) scale += (long)m * scale_mstride;
  const int r0 = blockIdx.y * 64;
  const int c0 = blockIdx.x * 64;
  const int t = threadIdx.x;

#pragma unroll
  for (int p = 0; p < 16; ++p) {
    int r = p * 4 + t / 64;
    int c = t % 64;
    float v = 0.f;
    if (r0 + r < R && c0 + c < C) {
      v = src[(long)(r0 + r) * C + c0 + c];
      if (scale) v *= scale[r0 + r];
    }
    tile[r][c] = v;
  }
  __syncthreads();
#pragma unroll
  for (int p = 0; p < 16; ++p) {
    int c = p * 4 + t / 64;  // output row (= source column)
    int r = t % 64;          // output col (= source row)
    if (c0 + c < C && r0 + r < R) dst[(long)(c0 + c) * R + r0 + r] = tile[r][c];
  }
}

// ---------------------------------------------------------------------------
// k_enc_fwd2_t: enc forward with PRE-TRANSPOSED operands (xT [d,B], WT [M,d,n],
// already inv-norm-scaled for tied) — both tiles stage DIRECT (b128 writes).
// ---------------------------------------------------------------------------
template <int TBK, int MINW, int TBN = BN>
__global__ __launch_bounds__(NTHREADS, MINW)
void k_enc_fwd2_t(const float* __restrict__ xT,      // [d, B]
                  const float* __restrict__ WT,      // [M, d, n]
                  const float* __restrict__ bias,    // [M, n]
                  float* __restrict__ c_out,         // [M, B, n]
                  float* __restrict__ loss_parts,    // [M, 2]
                  float* __restrict__ fired,         // [M, n]
                  int B, int d, int n, int mode, int prio,
                  const int* __restrict__ dict_sizes) {
  __shared__ DLds<TBK, BM> As;
  __shared__ DLds<TBK, TBN> Bs;

  constexpr int NACC = Tile<TBN>::NACC;
  Tile<TBN> t(prio);  // row0: batch rows, col0: dict cols
  const int m = t.m;
  const float* WT_m = WT + (long)m * d * n;

  DStage<TBK, BM> sa;
  DStage<TBK, TBN> sb;
  gemm_mainloop<TBK>(
      d, As, Bs, t.acc,
      [&](int k0) { stage_D_load<TBK, BM>(xT, B, k0, t.row0, d, B, nullptr, sa); },
      [&](int k0) { stage_D_load<TBK, TBN>(WT_m, n, k0, t.col0, d, n, nullptr, sb); },
      [&](int buf) { stage_D_write(sa, As, buf, false); },
      [&](int buf) { stage_D_write(sb, Bs, buf, false); });

  const EpiGeom g = epi_geom<NACC>();
  EpiIndex<false> ei(t.row0, t.col0, n, g);
  float* c_m = c_out + (long)m * B * n;
  const float* bias_m = bias + (long)m * n;
  float* fired_m = fired + (long)m * n;

  float l1_sum = 0.f;
  epi_cols<NACC, false>(g, t.col0, n, [&](int tj, int col, bool col_ok) {
    if (mode == ENC_RAW) {
      epi_rows<false>(g, ei, t.row0, B, tj, col, col_ok,
                      [&](int r, auto at) { at(c_m) = t.acc[tj][r]; });
      return;
    }
    float bj = col_ok ? bias_m[col] : 0.f;
    bool live = col_ok && (!dict_sizes || col < dict_sizes[m]);
    float fired_cnt = 0.f;
    epi_rows<false>(g, ei, t.row0, B, tj, col, col_ok, [&](int r, auto at) {
      float v = live ? fmaxf(t.acc[tj][r] + bj, 0.f) : 0.f;
      at(c_m) = v;
      l1_sum += v;
      fired_cnt += (v > 0.f) ? 1.f : 0.f;
    });
    float tot;
    if (col_ok && halfwave_pair_sum(g, fired_cnt, tot) && tot > 0.f) atomicAdd(&fired_m[col], tot);
  });
  if (mode == ENC_RELU) {
    l1_sum = wave_reduce_sum(l1_sum);
    if (g.lane == 0) atomicAdd(&loss_parts[m * 2 + 1], l1_sum);
  }
}

// ---------------------------------------------------------------------------
// k_gc2_t: code-grad with pre-transposed rT [M,d,B] and WT (scaled) [M,d,n].
// ---------------------------------------------------------------------------
template <int TBK, int MINW, int TBN = BN>
__global__ __launch_bounds__(NTHREADS, MINW)
void k_gc2_t(const float* __restrict__ rT,       // [M, d, B]
             const float* __restrict__ WT,       // [M, d, n] (inv-norm scaled)
             const float* __restrict__ c,        // [M, B, n]
             const float* __restrict__ l1_alpha, // [M]
             float* __restrict__ gpre_out,       // [M, B, n]
             float* __restrict__ g_bias,         // [M, n]
             int B, int d, int n, int prio, int gc_mode) {
  __shared__ DLds<TBK, BM> As;
  __shared__ DLds<TBK, TBN> Bs;

  constexpr int NACC = Tile<TBN>::NACC;
  Tile<TBN> t(prio);
  const int m = t.m;
  const float* rT_m = rT + (long)m * d * B;
  const float* WT_m = WT + (long)m * d * n;
  const float* c_m = c + (long)m * B * n;
  const float gscale = 2.0f / ((float)B * (float)d);
  const float l1_term = l1_alpha[m] / (float)B;

  DStage<TBK, BM> sa;
  DStage<TBK, TBN> sb;
  gemm_mainloop<TBK>(
      d, As, Bs, t.acc,
      [&](int k0) { stage_D_load<TBK, BM>(rT_m, B, k0, t.row0, d, B, nullptr, sa); },
      [&](int k0) { stage_D_load<TBK, TBN>(WT_m, n, k0, t.col0, d, n, nullptr, sb); },
      [&](int buf) { stage_D_write(sa, As, buf, false); },
      [&](int buf) { stage_D_write(sb, Bs, buf, false); });

  const EpiGeom g = epi_geom<NACC>();
  EpiIndex<false> ei(t.row0, t.col0, n, g);
  float* g_m = gpre_out + (long)m * B * n;
  float* gb_m = g_bias + (long)m * n;

  // default floating-point contraction here, unlike k_gc_t
  epi_cols<NACC, false>(g, t.col0, n, [&](int tj, int col, bool col_ok) {
    float colsum = 0.f;
    epi_rows<false>(g, ei, t.row0, B, tj, col, col_ok, [&](int r_, auto at) {
      float cv = at(c_m);
      float gv;
      if (gc_mode == GC_REVERSE) {
        float sgn = (cv > 0.f) ? 1.f : ((cv < 0.f) ? -1.f : 0.f);
        gv = (cv != 0.f) ? (gscale * t.acc[tj][r_] + l1_term * sgn) : 0.f;
      } else {
        gv = (cv > 0.f) ? (gscale * t.acc[tj][r_] + l1_term) : 0.f;
      }
      at(g_m) = gv;
      colsum += gv;
    });
    float tot;
    if (col_ok && gc_mode == GC_RELU && halfwave_pair_sum(g, colsum, tot) && tot != 0.f)
      atomicAdd(&gb_m[col], tot);
  });
}
