// The AuxK dead-latent loss of the TopK step (models/topk_auxk.py), d <= 2048.
// Included by sae_ops.hip behind sae_kernels.hip and sae_wsparse.hip, whose
// spk_*, sgw_* and wsp_below helpers it uses.
//
// Feature j of model m is dead when ages[m, j] >= dead_after[m].  Per row the
// kk = min(k_aux, n_dead) largest positive scores over the dead columns make
// the aux code z; e_hat = z @ What is held against e = x - x_hat = -r, and the
// gradient of alpha * mean((e_hat - e)^2) is added to the main chain's gw.
//
//   k_auxk_age      n_dead[m] from the ages (head of the step), or the ages'
//                   update from the main chain's hit_counts (end of the step)
//   k_auxk_select   one workgroup per (model, row): exact radix select over the
//                   dead columns, output compact and ascending in column
//   k_auxk_dec_gc   one wave per row: r_aux = z @ What + r, its squares into
//                   loss_parts[m, 1], gpre_aux at the list's entries
//   k_auxk_grad_w   one workgroup per (model, strip of 64 features):
//                   gw[j, :] += sum over the hit rows of gs val r_aux + gpre_aux x
//
// A model with n_dead == 0 or k_aux == 0 is idle: every workgroup of the last
// three kernels leaves at once (the select stores the row's count of 0), so
// loss_parts[m, 1] stays the exact 0 the step wrote and gw the main chain's bits.
//
// As in the sparse chain: SPK_NOPK and builtins only (no call, no packed fp32),
// no float atomic but the one per block into the loss partial, and every sum in
// an order fixed by the inputs alone: r_aux, gpre_aux and gw are reproducible
// bit for bit.
//
// Where this departs from a feature-major list build (k_sparse_grad_w's phase
// 1): the aux code exists only as compact row lists, so a feature's hit rows
// are not found by reading a column.  k_auxk_grad_w walks the batch in windows
// of AXG_WIN rows instead.  Per window every row finds the strip's entries in
// its ascending list by binary search and drops slot + 1 into an LDS table
// [feature][row of the window]; a wave then reads a feature's table row with
// ballots, which yields its hits in ascending row order with no list, no
// workspace and no capacity.  A feature's window sum is added into gw at the
// window's end by the one wave that owns the feature, so the order of gw's
// sums is: windows ascending, rows ascending inside.
//
// Registers, scratch and LDS per instantiation, from the gfx950 code object's
// metadata (.vgpr_count / .private_segment_fixed_size /
// .group_segment_fixed_size); no variant spills:
//
//   DL                       1    2    4    8   12   16   32
//   k_auxk_dec_gc   VGPRs   18   18   20   30   42   56  119   (8 waves/SIMD asked for; 2 at DL = 32)
//   k_auxk_grad_w   VGPRs   26   27   39   63   87  112  225   (4 waves/SIMD asked for; 2 at DL = 32)
//   scratch bytes (both)     0    0    0    0    0    0    0
//   LDS bytes: k_auxk_dec_gc 16, k_auxk_grad_w 32768 (the window table)
//   k_auxk_age     8 VGPRs, no scratch,   16 B LDS
//   k_auxk_select 24 VGPRs, no scratch, 1072 B LDS

#define AXA_T 256              // k_auxk_age
#define AXS_T 256              // k_auxk_select
#define AXS_NW (AXS_T / WAVE)
#define AXG_WIN 256            // k_auxk_grad_w: rows per window
#define AUXK_MAX_D SPARSE_MAX_D
#define AUXK_MAX_KA 65534      // slot + 1 fits the table's 16 bits

static_assert(AXG_WIN <= SGW_T && AXG_WIN % WAVE == 0, "one thread per row of a window");

SPK_DEV bool axk_idle(const int* __restrict__ n_dead, const int* __restrict__ k_aux, int m) {
  return n_dead[m] <= 0 || k_aux[m] <= 0;
}

SPK_DEV unsigned axk_ord(float f) {  // f32_ord
  const unsigned u = __builtin_bit_cast(unsigned, f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// a list's column, kept inside the dictionary whatever the list holds
SPK_DEV int axk_col(const int* __restrict__ idx, int i, int n) {
  const int j = __builtin_amdgcn_readfirstlane(idx[i]);
  return j < 0 ? 0 : spk_min(j, n - 1);
}

// ---------------------------------------------------------------------------
// k_auxk_age: grid (M); block AXA_T.
// update == 0: n_dead[m] = #{j : ages[m, j] >= dead_after[m]} (ballots, the
//   waves' counts through LDS: integers, any order).
// update == 1: ages[m, j] = hit_counts[m, j] > 0 ? 0 : ages[m, j] + 1, held at
//   INT_MAX.  hit_counts is the main chain's "c[:, j] > 0 on some row".
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(AXA_T) SPK_NOPK
void k_auxk_age(int* __restrict__ ages,              // [M, n]
                const int* __restrict__ hit_counts,  // [M, n]; read at update == 1
                const int* __restrict__ dead_after,  // [M]
                int* __restrict__ n_dead,            // [M]; written at update == 0
                int n, int update) {
  __shared__ int wave_cnt[AXA_T / WAVE];
  const int lane = spk_tid() & (WAVE - 1);
  const int wave = spk_wave_id();
  const int m = (int)__builtin_amdgcn_workgroup_id_x();
  int* age = ages + (long)m * n;
  if (update) {
    const int* hc = hit_counts + (long)m * n;
    for (int j = spk_tid(); j < n; j += AXA_T) {
      const int a = age[j];
      age[j] = hc[j] > 0 ? 0 : (a < 0x7fffffff ? a + 1 : a);
    }
    return;
  }
  const int da = dead_after[m];
  int k = 0;
  for (int j0 = 0; j0 < n; j0 += AXA_T) {
    const int j = j0 + spk_tid();
    k += __builtin_popcountll(spk_ballot(j < n && age[j < n ? j : 0] >= da));
  }
  if (lane == 0) wave_cnt[wave] = k;
  spk_barrier();
  if (spk_tid() == 0) n_dead[m] = (wave_cnt[0] + wave_cnt[1]) + (wave_cnt[2] + wave_cnt[3]);
}

// ---------------------------------------------------------------------------
// k_auxk_select: grid (B, M); block AXS_T.  The candidates of row b are the
// columns j with ages[m, j] >= dead_after[m] and S[b, j] > 0 (a NaN is none).
// Pass by pass (8 bits, MSB first) an LDS histogram of the candidates' f32_ord
// keys that match the prefix decided so far gives the key thr of the kk-th
// largest candidate and the number of ties at thr still to take; integer LDS
// atomics, so the counts do not depend on their order.  With at most kk
// candidates (seen in the first pass's total) all are taken.
// The write pass goes over the columns in ascending order, 256 per round, a
// wave on 64 consecutive ones.  A column is taken if its key is above thr, or
// equal and fewer than `ties` equal ones lie below it: that rank, and then the
// output position, are the running total, the lower waves' counts (LDS) and
// the ballot's bits below the lane.  So the lowest columns win a tie, and
// aux_idx[m, b, 0 .. cnt) ascends.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(AXS_T) SPK_NOPK
void k_auxk_select(const float* __restrict__ scores,    // [M, B, n]
                   const int* __restrict__ ages,        // [M, n]
                   const int* __restrict__ dead_after,  // [M]
                   const int* __restrict__ k_aux,       // [M]
                   const int* __restrict__ n_dead,      // [M]
                   int* __restrict__ aux_idx,           // [M, B, KA]
                   float* __restrict__ aux_val,         // [M, B, KA]
                   int* __restrict__ aux_cnt,           // [M, B]
                   int B, int n, int KA) {
  __shared__ unsigned hist[256];
  __shared__ unsigned sh_prefix, sh_mask, sh_kleft, sh_all;
  __shared__ int wcnt[2][AXS_NW];
  const int tid = spk_tid();
  const int lane = tid & (WAVE - 1);
  const int wave = spk_wave_id();
  const int m = (int)__builtin_amdgcn_workgroup_id_y();
  const long row = (long)m * B + (int)__builtin_amdgcn_workgroup_id_x();
  if (axk_idle(n_dead, k_aux, m)) {
    if (tid == 0) aux_cnt[row] = 0;
    return;
  }
  const int kk = spk_min(spk_min(k_aux[m], n_dead[m]), KA);
  const float* s = scores + row * n;
  const int* age = ages + (long)m * n;
  const int da = dead_after[m];

  if (tid == 0) {
    sh_prefix = 0u;
    sh_mask = 0u;
    sh_kleft = (unsigned)kk;
    sh_all = 0u;
  }
  spk_barrier();
  for (int shift = 24; shift >= 0; shift -= 8) {
    hist[tid] = 0u;
    spk_barrier();
    const unsigned prefix = sh_prefix, mask = sh_mask;
    for (int j = tid; j < n; j += AXS_T) {
      const float v = s[j];
      if (v > 0.f && age[j] >= da) {
        const unsigned u = axk_ord(v);
        if ((u & mask) == prefix)
          __hip_atomic_fetch_add(&hist[(u >> shift) & 0xFFu], 1u, __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_WORKGROUP);
      }
    }
    spk_barrier();
    if (tid == 0) {
      unsigned kleft = sh_kleft;
      bool all = false;
      if (shift == 24) {
        unsigned total = 0u;
        for (int bin = 0; bin < 256; ++bin) total += hist[bin];
        all = total <= kleft;
      }
      if (all) {  // every candidate: all keys are above 0
        sh_all = 1u;
        sh_kleft = 0u;
      } else {
        int bin = 255;
        for (; bin > 0; --bin) {
          if (hist[bin] >= kleft) break;
          kleft -= hist[bin];
        }
        sh_kleft = kleft;
        sh_prefix = prefix | ((unsigned)bin << shift);
        sh_mask = mask | (0xFFu << shift);
      }
    }
    spk_barrier();
    if (sh_all) break;  // uniform
  }

  const unsigned thr = sh_prefix;
  const int ties = (int)sh_kleft;
  int* idx = aux_idx + row * KA;
  float* val = aux_val + row * KA;
  int run_eq = 0, run_sel = 0;
  for (int j0 = 0; j0 < n; j0 += AXS_T) {
    const int j = j0 + tid;
    const bool in = j < n;
    const float v = in ? s[j] : 0.f;
    const bool cand = in && v > 0.f && age[in ? j : 0] >= da;
    const unsigned u = axk_ord(v);
    const bool eq = cand && u == thr;
    const unsigned long long eqb = spk_ballot(eq);
    if (lane == 0) wcnt[0][wave] = __builtin_popcountll(eqb);
    spk_barrier();
    int off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < AXS_NW; ++w) {
      const int k = wcnt[0][w];
      off += w < wave ? k : 0;
      tot += k;
    }
    const bool sel = (cand && u > thr) || (eq && run_eq + off + wsp_below(eqb) < ties);
    const unsigned long long selb = spk_ballot(sel);
    if (lane == 0) wcnt[1][wave] = __builtin_popcountll(selb);
    spk_barrier();  // also: every wave has read wcnt[0] of this round
    int off2 = 0, tot2 = 0;
#pragma unroll
    for (int w = 0; w < AXS_NW; ++w) {
      const int k = wcnt[1][w];
      off2 += w < wave ? k : 0;
      tot2 += k;
    }
    const int pos = run_sel + off2 + wsp_below(selb);
    if (sel && pos < KA) {
      idx[pos] = j;
      val[pos] = v;
    }
    run_eq += tot;
    run_sel += tot2;
  }
  if (tid == 0) aux_cnt[row] = spk_min(run_sel, KA);
}

// ---------------------------------------------------------------------------
// k_auxk_dec_gc: one wave owns one batch row of one model, in k_sparse_dec_gc's
// register layout.  grid (ceil(B / 4), M); block SDG_T.
// Pass 0 walks the row's list in ascending column order, two rows of W in
// flight: acc = fma(val inv[j], W[j, :], acc).  r_aux = acc + r (e = -r) is
// stored and its squares are summed as k_sparse_dec_gc sums r's, one atomicAdd
// per block into loss_parts[m, 1].  Pass 1: gpre_aux[b, i] = (gs inv[j])
// dot(r_aux, W[j, :]) at the list's entry i, gs = alpha[m] 2 / (B d).
// A row without an entry stores r_aux = r and counts its squares.
// ---------------------------------------------------------------------------
template <int DL>
SPK_DEV void axk_load_row(float (&w)[DL], const float* __restrict__ wr, int d, int lane) {
#pragma unroll
  for (int i = 0; i < DL; ++i) {
    const int col = lane + i * WAVE;
    w[i] = col < d ? wr[col] : 0.f;
  }
}

template <int DL, int MINW>
__global__ __launch_bounds__(SDG_T, MINW) SPK_NOPK
void k_auxk_dec_gc(const int* __restrict__ aux_idx,      // [M, B, KA]
                   const float* __restrict__ aux_val,    // [M, B, KA]
                   const int* __restrict__ aux_cnt,      // [M, B]
                   const float* __restrict__ Wdec,       // [M, n, d]
                   const float* __restrict__ inv_norms,  // [M, n]
                   const float* __restrict__ r,          // [M, B, d], the main pass's
                   const float* __restrict__ alpha,      // [M]
                   const int* __restrict__ k_aux,        // [M]
                   const int* __restrict__ n_dead,       // [M]
                   float* __restrict__ r_aux,            // [M, B, d]
                   float* __restrict__ gpre_aux,         // [M, B, KA], written at the entries only
                   float* __restrict__ loss_parts,       // [M, 2]
                   int B, int d, int n, int KA) {
  __shared__ float wave_ss[SDG_T / WAVE];
  const int lane = spk_tid() & (WAVE - 1);
  const int wave = spk_wave_id();
  const int m = (int)__builtin_amdgcn_workgroup_id_y();
  if (axk_idle(n_dead, k_aux, m)) return;  // the whole block
  const int b = (int)__builtin_amdgcn_workgroup_id_x() * (SDG_T / WAVE) + wave;

  float ss = 0.f;
  if (b < B) {
    const long row = (long)m * B + b;
    const int cnt = spk_min(__builtin_amdgcn_readfirstlane(aux_cnt[row]), KA);
    const int* idx = aux_idx + row * KA;
    const float* val = aux_val + row * KA;
    const float* W = Wdec + (long)m * n * d;
    const float* inv = inv_norms + (long)m * n;
    const float gs = alpha[m] * (2.0f / ((float)B * (float)d));

    float acc[DL];
#pragma unroll
    for (int i = 0; i < DL; ++i) acc[i] = 0.f;
    int h = 0;
    for (; h + 1 < cnt; h += 2) {
      const int ja = axk_col(idx, h, n), jb = axk_col(idx, h + 1, n);
      const float sa = val[h] * inv[ja], sb = val[h + 1] * inv[jb];
      float wa[DL], wb[DL];
      axk_load_row<DL>(wa, W + (long)ja * d, d, lane);
      axk_load_row<DL>(wb, W + (long)jb * d, d, lane);
#pragma unroll
      for (int i = 0; i < DL; ++i) acc[i] = __builtin_fmaf(sa, wa[i], acc[i]);
#pragma unroll
      for (int i = 0; i < DL; ++i) acc[i] = __builtin_fmaf(sb, wb[i], acc[i]);
    }
    if (h < cnt) {
      const int ja = axk_col(idx, h, n);
      const float sa = val[h] * inv[ja];
      float wa[DL];
      axk_load_row<DL>(wa, W + (long)ja * d, d, lane);
#pragma unroll
      for (int i = 0; i < DL; ++i) acc[i] = __builtin_fmaf(sa, wa[i], acc[i]);
    }
    const float* rrow = r + row * d;
    float* arow = r_aux + row * d;
#pragma unroll
    for (int i = 0; i < DL; ++i) {
      const int col = lane + i * WAVE;
      float rv = 0.f;  // columns past d stay 0 for the dots of pass 1
      if (col < d) {
        rv = acc[i] + rrow[col];
        arow[col] = rv;
      }
      acc[i] = rv;
      ss = __builtin_fmaf(rv, rv, ss);
    }
    ss = spk_wave_sum(ss, lane);

    float* grow = gpre_aux + row * KA;
    for (h = 0; h < cnt; ++h) {
      const int j = axk_col(idx, h, n);
      float w[DL];
      axk_load_row<DL>(w, W + (long)j * d, d, lane);
      float dot = 0.f;
#pragma unroll
      for (int i = 0; i < DL; ++i) dot = __builtin_fmaf(acc[i], w[i], dot);
      dot = spk_wave_sum(dot, lane);
      if (lane == 0) grow[h] = (gs * inv[j]) * dot;
    }
  }
  if (lane == 0) wave_ss[wave] = ss;
  spk_barrier();
  if (spk_tid() == 0)
    __hip_atomic_fetch_add(&loss_parts[m * 2 + 1],
                           (wave_ss[0] + wave_ss[1]) + (wave_ss[2] + wave_ss[3]),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------------------
// k_auxk_grad_w: grid (ceil(n / 64), M); block SGW_T = 8 waves.  A strip
// without a dead column leaves at once (a ballot over its ages, the same in
// every wave).  Per window of AXG_WIN rows:
//   clear   the table tab[f][w] (16 bits: slot + 1, 0 for no hit), 32 KB
//   fill    thread w < AXG_WIN owns row b0 + w: the first entry of its
//           ascending list with column >= j0 by binary search, then the entries
//           below j0 + 64: tab[col - j0][w] = slot + 1.  A row holds a column
//           once, so no two threads store to one cell.
//   sum     the strip's dead features go round the waves.  A wave reads its
//           feature's table row 64 cells at a time; the ballot's set bits in
//           ascending order are the feature's hit rows of the window, the cell
//           the slot of val and gpre_aux.  Per hit k_sparse_grad_w's two fmas
//           (sgw_load / sgw_apply with gs val for gscale c), two hits' loads in
//           flight.  A feature with a hit in the window then takes
//           gw[j, :] += acc: a plain load, add and store, since the main
//           chain's launch completed gw and no other wave touches the row.
// ---------------------------------------------------------------------------
template <int DL>
SPK_DEV void axg_hit(SgwHit<DL>& h, int cell, int b, long m_rows, const float* __restrict__ aux_val,
                     const float* __restrict__ gpre_aux, const float* __restrict__ ra_m,
                     const float* __restrict__ x_m, float gs, int KA, int d, int lane) {
  const long at = m_rows * KA + (cell - 1);  // + b * KA inside sgw_load
  sgw_load<DL>(h, b, aux_val + at, gpre_aux + at, ra_m, x_m, gs, KA, d, d, lane);
}

template <int DL, int MINW>
__global__ __launch_bounds__(SGW_T, MINW) SPK_NOPK
void k_auxk_grad_w(const int* __restrict__ aux_idx,      // [M, B, KA]
                   const float* __restrict__ aux_val,    // [M, B, KA]
                   const int* __restrict__ aux_cnt,      // [M, B]
                   const float* __restrict__ gpre_aux,   // [M, B, KA]
                   const float* __restrict__ r_aux,      // [M, B, d]
                   const float* __restrict__ x,          // [B, d] or [M, B, d]
                   const int* __restrict__ ages,         // [M, n]
                   const int* __restrict__ dead_after,   // [M]
                   const int* __restrict__ k_aux,        // [M]
                   const int* __restrict__ n_dead,       // [M]
                   const float* __restrict__ alpha,      // [M]
                   float* gw,                            // [M, n, d], added into
                   int B, int d, int n, int KA, long x_mstride) {
  __shared__ unsigned short tab[SGW_STRIP][AXG_WIN];
  const int tid = spk_tid();
  const int lane = tid & (WAVE - 1);
  const int wave = spk_wave_id();
  const int m = (int)__builtin_amdgcn_workgroup_id_y();
  const int j0 = (int)__builtin_amdgcn_workgroup_id_x() * SGW_STRIP;
  if (axk_idle(n_dead, k_aux, m)) return;
  const int jl = j0 + lane;
  const unsigned long long dead =
      spk_ballot(jl < n && ages[(long)m * n + (jl < n ? jl : 0)] >= dead_after[m]);
  if (dead == 0ull) return;  // the same in every wave

  const long m_rows = (long)m * B;
  const float* ra_m = r_aux + m_rows * d;
  const float* x_m = x + (long)m * x_mstride;
  float* gw_m = gw + (long)m * n * d;
  const float gs = alpha[m] * (2.0f / ((float)B * (float)d));
  const int jend = spk_min(j0 + SGW_STRIP, n);

  for (int b0 = 0; b0 < B; b0 += AXG_WIN) {
    spk_barrier();  // the last window's readers are done
    for (int i = tid; i < SGW_STRIP * AXG_WIN; i += SGW_T) (&tab[0][0])[i] = 0;
    spk_barrier();
    if (tid < AXG_WIN && b0 + tid < B) {
      const long row = m_rows + b0 + tid;
      const int cnt = spk_min(aux_cnt[row], KA);
      const int* idx = aux_idx + row * KA;
      int lo = 0, hi = cnt;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (idx[mid] < j0) lo = mid + 1; else hi = mid;
      }
      for (; lo < cnt; ++lo) {
        const int j = idx[lo];
        if (j < j0 || j >= jend) break;  // j < j0: not an ascending list
        tab[j - j0][tid] = (unsigned short)(lo + 1);
      }
    }
    spk_barrier();

    float acc[DL];
    for (int f = wave; j0 + f < jend; f += SGW_NW) {
      if (!((dead >> f) & 1ull)) continue;
      bool any = false;
      for (int w0 = 0; w0 < AXG_WIN; w0 += WAVE) {
        const int cell = tab[f][w0 + lane];
        unsigned long long hit = spk_ballot(cell != 0);
        if (hit && !any) {
          any = true;
#pragma unroll
          for (int i = 0; i < DL; ++i) acc[i] = 0.f;
        }
        while (hit) {
          const int La = __builtin_ctzll(hit);
          hit &= hit - 1;
          SgwHit<DL> ha;
          axg_hit<DL>(ha, __builtin_amdgcn_readlane(cell, La), b0 + w0 + La, m_rows, aux_val, gpre_aux,
                      ra_m, x_m, gs, KA, d, lane);
          if (hit) {
            const int Lb = __builtin_ctzll(hit);
            hit &= hit - 1;
            SgwHit<DL> hb;
            axg_hit<DL>(hb, __builtin_amdgcn_readlane(cell, Lb), b0 + w0 + Lb, m_rows, aux_val, gpre_aux,
                        ra_m, x_m, gs, KA, d, lane);
            sgw_apply<DL>(acc, ha);
            sgw_apply<DL>(acc, hb);
          } else {
            sgw_apply<DL>(acc, ha);
          }
        }
      }
      if (any) {
        float* grow = gw_m + (long)(j0 + f) * d;
#pragma unroll
        for (int i = 0; i < DL; ++i) {
          const int col = lane + i * WAVE;
          if (col < d) grow[col] += acc[i];
        }
      }
    }
  }
}
