// The wide split of the sparse TopK and Matryoshka chains: 2048 < d <= 8192.
// Included by sae_ops.hip behind sae_kernels.hip, whose spk_*, sgw_* and msp_*
// helpers it uses.
//
// The narrow kernels (sae_kernels.hip) keep a whole length-d vector in one
// wave, DL = ceil(d / 64) registers per lane, and stop at DL = 32.  Here the
// vector is split over the eight waves of a workgroup instead:
//
//   k_wsparse_dec_gc    one workgroup per batch row; the row's hits are
//                       compacted into an LDS list once and every wave walks
//                       that list over its own columns
//   k_sparse_hit_lists  k_sparse_grad_w's phase 1 (the per-feature hit lists)
//                       as a launch of its own
//   k_wsparse_grad_w    k_sparse_grad_w's phase 2 per window of 1024 columns,
//                       reading those lists
//
// All three are level-aware (G nested prefixes, as the narrow kernels' LEVELS
// instantiations); the plain chain is G = 1 with R = r.  A column's sums run in the order of the
// narrow kernels (ascending features for r, ascending hit rows for gw, the same
// light/heavy rule), so a column of r or gw holds the bits a narrow launch on
// that column gives.  Only gpre's dot and the loss are reduced differently:
// they span eight waves.  No float atomics feed r, S, gpre or gw.
//
// Registers, scratch and LDS per instantiation, from the gfx950 code object's
// metadata (.vgpr_count / .private_segment_fixed_size /
// .group_segment_fixed_size).  Waves per SIMD are what the launch bounds ask
// for and the VGPR counts allow (512 / VGPRs, in whole 8-wave workgroups of
// 2 waves per SIMD each): derived, not observed on a device.
//
//   kernel                      VGPRs  scratch  LDS bytes  waves/SIMD
//   k_wsparse_dec_gc   DLW = 8    67      0      33120     4 asked for; 6 (three workgroups; LDS lets four in)
//   k_wsparse_dec_gc   DLW = 16  124      0      33120     4 asked for; 4
//   k_sparse_hit_lists            25      0       2048     8
//   k_wsparse_grad_w   DL = 16   122      0      33024     2 asked for (see the kernel); 4

#define WSP_T 512              // 8 waves: wave w, register i, lane l own column (i * 8 + w) * 64 + l
#define WSP_NW (WSP_T / WAVE)
#define WSP_CAP 2048           // entries of the LDS hit list: 8 KB of indices, 8 KB of scales
#define WSP_GROUP 8            // hits whose dots go through LDS together, one per wave
#define WSP_MAX_DLW 16
#define WSPARSE_MAX_D (WSP_MAX_DLW * WSP_T)  // 8192
#define WSGW_DL 16             // k_wsparse_grad_w: registers per lane and window
#define WSGW_CHUNK (WSGW_DL * WAVE)          // 1024 columns per window

static_assert(WSP_NW == 8 && WSP_GROUP == WSP_NW, "one wave sums one hit of a group");
static_assert(4 * WSP_T <= WSP_CAP, "an empty list must take any one round of the scan");
static_assert(WSGW_CHUNK == SGW_CW_MAX, "a window is combined through LDS in one round");

struct WspLds {
  int j[WSP_CAP];                   // the hits' features, ascending
  float s[WSP_CAP];                 // c[b, j] * inv[j]
  float part[WSP_GROUP][WSP_T];     // pass 1: lane partials of a group's dots
  int wcnt[2][WSP_NW];              // the waves' hit counts of a round, by the round's parity
  int level_hi[MSP_MAX_G];          // list index behind level g's last hit (single fill only)
  float wave_ss[MSP_MAX_G][WSP_NW];
};

SPK_DEV int wsp_below(unsigned long long mask) {  // set bits of mask below this lane
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32),
                                        __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

// The row is scanned in rounds.  Where its base is 16-byte aligned, the columns
// below nvec = n & ~3 go 8 x 256 per round (a float4 and a 4-bit mask per lane,
// the narrow kernel's scan); the rest, or the whole row where nvec is 0, goes
// 8 x 64 per round.  The first column of the round that holds column `col`:
SPK_DEV int wsp_round_of(int col, int nvec) {
  return col < nvec ? col & ~(4 * WSP_T - 1) : nvec + ((col - nvec) & ~(WSP_T - 1));
}

// Compacts the hits `c > 0` of the columns [jlo, jhi) into the list, ascending,
// from the round at j0 on, and returns their number.  A round that does not
// fit is left for the next call (an empty list takes any round); j0 is the
// first round not taken, j0 >= jhi when the columns are done.  A lane's place:
// the hits already listed, the hits of the waves below (their counts go
// through LDS), the hits of the lanes below (popcount of the four ballots
// below the lane), the hits of its own nibble below.  Every branch on the way
// is uniform over the workgroup.
SPK_DEV int wsp_fill(WspLds& L, const float* __restrict__ crow, const float* __restrict__ inv,
                     int nvec, int& j0, int jlo, int jhi, int lane, int wave) {
  spk_barrier();  // the list's readers are done with it
  int count = 0, par = 0;
  while (j0 < jhi) {
    const bool vec = j0 < nvec;
    const int step = vec ? 4 : 1;
    const int col = j0 + step * (wave * WAVE + lane);
    spk_f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (vec) {
      if (col < nvec) v = *reinterpret_cast<const spk_f32x4*>(crow + col);
    } else if (col < jhi) {
      v.x = crow[col];
    }
    // columns col + q, q > 0, exist only in a float4 round, where col + 3 < nvec
    const int nib = (v.x > 0.f && col >= jlo && col < jhi ? 1 : 0) |
                    (v.y > 0.f && col + 1 >= jlo && col + 1 < jhi ? 2 : 0) |
                    (v.z > 0.f && col + 2 >= jlo && col + 2 < jhi ? 4 : 0) |
                    (v.w > 0.f && col + 3 >= jlo && col + 3 < jhi ? 8 : 0);
    const unsigned long long b0 = spk_ballot(nib & 1), b1 = spk_ballot(nib & 2);
    const unsigned long long b2 = spk_ballot(nib & 4), b3 = spk_ballot(nib & 8);
    const int below = wsp_below(b0) + wsp_below(b1) + wsp_below(b2) + wsp_below(b3);
    const int wtot = __builtin_popcountll(b0) + __builtin_popcountll(b1) +
                     __builtin_popcountll(b2) + __builtin_popcountll(b3);
    if (lane == 0) L.wcnt[par][wave] = wtot;
    spk_barrier();
    int off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < WSP_NW; ++w) {
      const int k = L.wcnt[par][w];
      off += w < wave ? k : 0;
      tot += k;
    }
    if (count + tot > WSP_CAP) break;
    int p = count + off + below;
    if (nib & 1) { L.j[p] = col;     L.s[p] = v.x * inv[col];     ++p; }
    if (nib & 2) { L.j[p] = col + 1; L.s[p] = v.y * inv[col + 1]; ++p; }
    if (nib & 4) { L.j[p] = col + 2; L.s[p] = v.z * inv[col + 2]; ++p; }
    if (nib & 8) { L.j[p] = col + 3; L.s[p] = v.w * inv[col + 3]; }
    count += tot;
    j0 = vec ? spk_min(j0 + 4 * WSP_T, nvec) : j0 + WSP_T;
    par ^= 1;  // a wave a round ahead writes the other row of wcnt
  }
  spk_barrier();
  return count;
}

// first index in [lo, hi) of the ascending L.j whose feature is >= e, or hi
SPK_DEV int wsp_first_at(const WspLds& L, int lo, int hi, int e) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (L.j[mid] < e) lo = mid + 1; else hi = mid;
  }
  return lo;
}

template <int DLW>
SPK_DEV void wsp_load_row(float (&w)[DLW], const float* __restrict__ wr, int d, int col0) {
#pragma unroll
  for (int i = 0; i < DLW; ++i) {
    const int col = col0 + i * WSP_T;
    w[i] = col < d ? wr[col] : 0.f;
  }
}

// pass 0: acc += s * W[j, :] over the list's entries [h, hi), ascending; the
// index and the scale are wave-uniform, two rows' loads in flight
template <int DLW>
SPK_DEV void wsp_walk(float (&acc)[DLW], const WspLds& L, int h, int hi,
                      const float* __restrict__ W, int d, int col0) {
  for (; h + 1 < hi; h += 2) {
    const int ja = __builtin_amdgcn_readfirstlane(L.j[h]);
    const int jb = __builtin_amdgcn_readfirstlane(L.j[h + 1]);
    const float sa = L.s[h], sb = L.s[h + 1];
    float wa[DLW], wb[DLW];
    wsp_load_row<DLW>(wa, W + (long)ja * d, d, col0);
    wsp_load_row<DLW>(wb, W + (long)jb * d, d, col0);
#pragma unroll
    for (int i = 0; i < DLW; ++i) acc[i] = __builtin_fmaf(sa, wa[i], acc[i]);
#pragma unroll
    for (int i = 0; i < DLW; ++i) acc[i] = __builtin_fmaf(sb, wb[i], acc[i]);
  }
  if (h < hi) {
    const int ja = __builtin_amdgcn_readfirstlane(L.j[h]);
    const float sa = L.s[h];
    float wa[DLW];
    wsp_load_row<DLW>(wa, W + (long)ja * d, d, col0);
#pragma unroll
    for (int i = 0; i < DLW; ++i) acc[i] = __builtin_fmaf(sa, wa[i], acc[i]);
  }
}

// pass 1: gpre[b, j] = (gscale inv[j]) dot(S, W[j, :]) at the list's entries
// [lo, hi).  The dot spans the workgroup, so the hits go in groups of 8: every
// thread leaves its partial (DLW fmas, ascending registers) of hit h in
// part[h][tid]; behind one barrier wave h sums hit h, a lane adding the 8
// waves' partials of its lane in ascending wave order, then the xor tree.  One
// tree per hit, and an order fixed by the shape alone.
template <int DLW>
SPK_DEV void wsp_gpre(const float (&S)[DLW], WspLds& L, int lo, int hi, const float* __restrict__ W,
                      const float* __restrict__ inv, float* __restrict__ gpre_row, float gscale,
                      int d, int col0, int lane, int wave) {
  for (int h0 = lo; h0 < hi; h0 += WSP_GROUP) {
    const int ng = spk_min(WSP_GROUP, hi - h0);
    for (int hh = 0; hh < ng; ++hh) {
      const int j = __builtin_amdgcn_readfirstlane(L.j[h0 + hh]);
      float w[DLW];
      wsp_load_row<DLW>(w, W + (long)j * d, d, col0);
      float dot = 0.f;
#pragma unroll
      for (int i = 0; i < DLW; ++i) dot = __builtin_fmaf(S[i], w[i], dot);
      L.part[hh][spk_tid()] = dot;
    }
    spk_barrier();
    if (wave < ng) {
      float dot = L.part[wave][lane];
#pragma unroll
      for (int w = 1; w < WSP_NW; ++w) dot += L.part[wave][w * WAVE + lane];
      dot = spk_wave_sum(dot, lane);
      if (lane == 0) {
        const int j = L.j[h0 + wave];
        gpre_row[j] = (gscale * inv[j]) * dot;
      }
    }
    spk_barrier();  // part is free for the next group
  }
}

// ---------------------------------------------------------------------------
// k_wsparse_dec_gc: grid (B, M); block WSP_T.  DLW registers per lane hold the
// thread's columns col0 + 512 i of the row: 8 for d <= 4096, 16 for d <= 8192.
// The interleaving keeps all eight waves at work at a d that does not fill the
// depth.
//
// Pass 0 fills the list from the row (wsp_fill) and walks it; at a level's end
// e_g the walk stops at the first entry with j >= e_g, r_g = acc - x goes to
// R[m, g, b, :] and its squares to the level's sum, and the walk goes on into
// the SAME accumulators, as k_sparse_dec_gc's does.  A row with more than
// WSP_CAP hits fills, consumes and refills the list; nothing assumes k.
// Pass 1 goes down from g = G-1 with S_g in the registers (msp_level_down).  Where the row fitted one
// fill, the normal case, the list is still whole and level g's entries are
// [level_hi[g-1], level_hi[g]): c is not read again.  Otherwise level g's
// columns are rescanned, fill by fill.
// Loss: lane, wave tree, the 8 waves through LDS in ascending order, one
// atomicAdd per workgroup and level into parts[m * parts_stride + g].
// ---------------------------------------------------------------------------
template <int DLW, int MINW>
__global__ __launch_bounds__(WSP_T, MINW) SPK_NOPK
void k_wsparse_dec_gc(const float* __restrict__ c,          // [M, B, n]
                      const float* __restrict__ Wdec,       // [M, n, d]
                      const float* __restrict__ inv_norms,  // [M, n]
                      const float* __restrict__ x,          // [B, d] or [M, B, d]
                      const int* __restrict__ ends,         // [M, G]; not read at G = 1
                      float* R,                             // [M, G, B, d]: r_g, then S_g
                      float* __restrict__ gpre,             // [M, B, n], written at the hits only
                      float* __restrict__ parts,            // level g of model m at m * parts_stride + g
                      int B, int d, int n, int G, long x_mstride, int parts_stride) {
  __shared__ WspLds L;
  const int lane = spk_tid() & (WAVE - 1);
  const int wave = spk_wave_id();
  const int col0 = wave * WAVE + lane;
  const int m = (int)__builtin_amdgcn_workgroup_id_y();
  const int b = (int)__builtin_amdgcn_workgroup_id_x();
  const int* ends_m = ends + (long)m * G;
  const float* crow = c + ((long)m * B + b) * n;
  const float* W = Wdec + (long)m * n * d;
  const float* inv = inv_norms + (long)m * n;
  const float* xrow = x + (long)m * x_mstride + (long)b * d;
  float* Rrow = R + ((long)m * G * B + b) * d;  // level g's row: + g * level
  const long level = (long)B * d;
  float* grow = gpre + ((long)m * B + b) * n;
  const float gscale = 2.0f / ((float)B * (float)d);
  const int nvec = (reinterpret_cast<uintptr_t>(crow) & 15) == 0 ? n & ~3 : 0;

  float acc[DLW];
#pragma unroll
  for (int i = 0; i < DLW; ++i) acc[i] = 0.f;
  bool one_fill = false;
  int j0 = 0, g = 0, e1 = msp_end(ends_m, 0, G, 0, n);
  for (int fills = 0; g < G; ++fills) {
    const int count = wsp_fill(L, crow, inv, nvec, j0, 0, n, lane, wave);
    const bool done = j0 >= n;
    one_fill = done && fills == 0;
    int h = 0;
    while (g < G) {
      const int hi = wsp_first_at(L, h, count, e1);
      wsp_walk<DLW>(acc, L, h, hi, W, d, col0);
      h = hi;
      if (h == count && !done) break;  // level g may go on in the next fill
      const float ss =
          msp_level_close<DLW, WSP_T>(acc, xrow, Rrow + g * level, g == G - 1, d, col0, lane);
      if (lane == 0) L.wave_ss[g][wave] = ss;
      if (spk_tid() == 0) L.level_hi[g] = h;
      ++g;
      if (g < G) e1 = msp_end(ends_m, g, G, e1, n);
    }
  }
  spk_barrier();  // level_hi

  for (g = G - 1; g >= 0; --g) {
    const int lo = msp_level_span(ends_m, g, G, n, e1);
    if (g < G - 1) msp_level_down<DLW, WSP_T>(acc, Rrow + g * level, d, col0);
    if (one_fill) {
      wsp_gpre<DLW>(acc, L, g ? L.level_hi[g - 1] : 0, L.level_hi[g], W, inv, grow, gscale, d, col0,
                    lane, wave);
    } else {
      int jr = wsp_round_of(lo, nvec);
      while (jr < e1) {
        const int count = wsp_fill(L, crow, inv, nvec, jr, lo, e1, lane, wave);
        wsp_gpre<DLW>(acc, L, 0, count, W, inv, grow, gscale, d, col0, lane, wave);
      }
    }
  }

  spk_barrier();  // wave_ss
  if (spk_tid() < G) {
    const float* ws = L.wave_ss[spk_tid()];
    float s = ws[0];
#pragma unroll
    for (int w = 1; w < WSP_NW; ++w) s += ws[w];
    __hip_atomic_fetch_add(&parts[(long)m * parts_stride + spk_tid()], s, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---------------------------------------------------------------------------
// k_sparse_hit_lists: k_sparse_grad_w's phase 1 alone.  grid (ceil(n / 64), M);
// block SGW_T.  Leaves hits[m, j, 0 .. count) and hit_counts[m, j] as that
// phase does; the end of the launch is what makes them visible to the launch
// behind it, where the narrow kernel needs its two fences.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(SGW_T) SPK_NOPK
void k_sparse_hit_lists(const float* __restrict__ c,   // [M, B, n]
                        int* __restrict__ hits,        // [M, n, B]
                        int* __restrict__ hit_counts,  // [M, n]
                        int B, int n) {
  __shared__ int cnt[SGW_NW][SGW_STRIP];
  const int m = (int)__builtin_amdgcn_workgroup_id_y();
  sgw_hit_lists((int)__builtin_amdgcn_workgroup_id_x() * SGW_STRIP, c + (long)m * B * n,
                hits + (long)m * n * B, hit_counts + (long)m * n, B, n, spk_lds(cnt),
                spk_tid() & (WAVE - 1), spk_wave_id());
}

// ---------------------------------------------------------------------------
// k_wsparse_grad_w: k_sparse_grad_w's phase 2 on one window of WSGW_CHUNK
// columns.  grid (ceil(n / 64), ceil(d / 1024), M); block SGW_T.  The phase is
// independent per column, so a window is sgw_strip_sums at DL = 16 with its row
// pointers moved to the window's first column and the window's width for d:
// the light/heavy rule and the order of every sum are the narrow kernel's.
// The launch bounds ask for 2 waves per SIMD, not the 4 that 128 registers
// allow: asked for 4, the compiler keeps 128 and spills 12 bytes; asked for 2,
// it takes the same 128 and spills nothing.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(SGW_T, 2) SPK_NOPK
void k_wsparse_grad_w(const float* __restrict__ c,             // [M, B, n]
                      const float* __restrict__ gpre,          // [M, B, n], read at the hits only
                      const float* __restrict__ R,             // [M, G, B, d]: S_g
                      const float* __restrict__ x,             // [B, d] or [M, B, d]
                      const int* __restrict__ ends,            // [M, G]; not read at G = 1
                      float* __restrict__ gw,                  // [M, n, d]
                      const int* __restrict__ hits,            // [M, n, B], from k_sparse_hit_lists
                      const int* __restrict__ hit_counts,      // [M, n]
                      int B, int d, int n, int G, long x_mstride) {
  __shared__ int tot[SGW_STRIP];
  __shared__ float part[SGW_NW][WSGW_CHUNK];

  const int lane = spk_tid() & (WAVE - 1);
  const int wave = spk_wave_id();
  const int m = (int)__builtin_amdgcn_workgroup_id_z();
  const int j0 = (int)__builtin_amdgcn_workgroup_id_x() * SGW_STRIP;
  const int c0 = (int)__builtin_amdgcn_workgroup_id_y() * WSGW_CHUNK;  // the window's first column
  const long level = (long)B * d;

  if (wave == 0) tot[lane] = j0 + lane < n ? hit_counts[(long)m * n + j0 + lane] : 0;
  spk_barrier();

  sgw_strip_sums<WSGW_DL>(spk_lds(tot), spk_lds(part), j0, hits + (long)m * n * B, c + (long)m * B * n,
                          gpre + (long)m * B * n, R + (long)m * G * level + c0, ends + (long)m * G,
                          x + (long)m * x_mstride + c0, gw + (long)m * n * d + c0, B, n, G, level,
                          2.0f / ((float)B * (float)d), d, spk_min(WSGW_CHUNK, d - c0), lane, wave);
}
