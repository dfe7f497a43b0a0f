// The JumpReLU step's two kernels (models/jumprelu.py), any d.
// Included by sae_ops.hip behind sae_kernels.hip, whose spk_* helpers it uses.
//
// Per model a threshold theta[n], a bandwidth eps and an L0 weight.  With the
// raw scores S = x @ What^T of k_enc_fwd (mode 1):
//
//   hit  [b, j] = S > theta[j] && S > 0          c = hit ? S : +0
//   band [b, j] = |S - theta[j]| < eps / 2       (fp32, one subtraction)
//
// Everything from c to gw is the sparse chain's (k_sparse_dec_gc,
// k_sparse_grad_w), which asks only for c > 0.  The threshold's gradient
//
//   g_theta[j] = -(1 / eps) sum_b band[b, j] (theta[j] g_f[b, j] + l0_alpha / B)
//   g_f[b, j]  = (2 / (B d)) inv[j] dot(r[b, :], W[j, :])
//
// runs over the band, which reaches below the threshold: those entries are no
// hits, the chain has no gpre for them, and the dot is computed here for every
// band entry alike.
//
//   k_jump_select      row-major: a workgroup takes JSL_ROWS rows of one model,
//                      a wave one group of 64 columns at a time.  It writes the
//                      dense c, the fired and L0 counts, and the band as one
//                      ballot word per (row, column group).
//   k_jump_grad_theta  feature-major: a workgroup owns a strip of 64 features
//                      of one model and walks the band words of its strip.
//
// The band travels as ballot words because the second kernel must not read the
// scores: k_sparse_grad_w reuses those bytes for its hit lists, and a word is
// 1/32 of the bytes of the scores it covers.  A strip whose band is empty costs
// k_jump_grad_theta one 8-byte load per row.
//
// As in the sparse chain: SPK_NOPK and builtins only, and no float atomic feeds
// c or g_theta.  g_theta's sums have an order fixed by the inputs alone (see
// k_jump_grad_theta), so it is reproducible bit for bit.  The counts are whole
// numbers, added with atomics in any order: fired in fp32 as k_topk_select's,
// l0_count in int32.

#define JSL_T 256                // k_jump_select
#define JSL_NW (JSL_T / WAVE)
#define JSL_ROWS 8               // rows per workgroup: one fired atomic per lane for all of them
#define JGT_T 512                // k_jump_grad_theta
#define JGT_NW (JGT_T / WAVE)
#define JGT_STRIP WAVE           // one band word wide

// ---------------------------------------------------------------------------
// k_jump_select: grid (ceil(B / JSL_ROWS), M); block JSL_T.  NW = ceil(n / 64)
// words per row.  Wave w takes the column groups w, w + JSL_NW, ...; per group
// lane l owns column 64 g + l over the workgroup's rows, so the scores are read
// and c is written 256 bytes per wave at a time, theta is read once, and the
// lane's hits over the rows go into fired[m, j] with one atomic.  Lanes past n
// take no part in a ballot.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(JSL_T) SPK_NOPK
void k_jump_select(const float* __restrict__ scores,          // [M, B, n]
                   const float* __restrict__ threshold,       // [M, n]
                   const float* __restrict__ bandwidth,       // [M]
                   float* __restrict__ c_out,                 // [M, B, n]
                   float* __restrict__ fired,                 // [M, n], added into
                   unsigned long long* __restrict__ band_bits,  // [M, B, NW]
                   int* __restrict__ l0_count,                // [M], added into
                   int B, int n, int NW) {
  const int lane = spk_tid() & (WAVE - 1);
  const int wave = spk_wave_id();
  const int m = (int)__builtin_amdgcn_workgroup_id_y();
  const int b0 = (int)__builtin_amdgcn_workgroup_id_x() * JSL_ROWS;
  const int b1 = spk_min(b0 + JSL_ROWS, B);
  const float half = 0.5f * bandwidth[m];
  const float* theta = threshold + (long)m * n;
  int hits = 0;  // wave-uniform
  for (int g = wave; g < NW; g += JSL_NW) {
    const int j = g * WAVE + lane;
    const bool in = j < n;
    const float th = in ? theta[j] : 0.f;
    int mine = 0;
    for (int b = b0; b < b1; ++b) {
      const long row = (long)m * B + b;
      const float s = in ? scores[row * n + j] : 0.f;
      const bool hit = in && s > th && s > 0.f;
      const bool bnd = in && __builtin_fabsf(s - th) < half;
      if (in) c_out[row * n + j] = hit ? s : 0.f;
      const unsigned long long bw = spk_ballot(bnd);
      if (lane == 0) band_bits[row * NW + g] = bw;
      hits += __builtin_popcountll(spk_ballot(hit));
      mine += hit ? 1 : 0;
    }
    if (mine > 0)
      __hip_atomic_fetch_add(&fired[(long)m * n + j], (float)mine, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
  }
  if (lane == 0 && hits > 0)
    __hip_atomic_fetch_add(&l0_count[m], hits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------------------
// k_jump_grad_theta: grid (NW, M); block JGT_T = 8 waves.  Strip s is the
// features 64 s .. 64 s + 63, the columns of band word s of every row.
//
// Wave w owns the rows b with b % 8 == w, ascending.  It takes 64 of them at a
// time: lane i loads the word of the i-th one, the words past n's last column
// masked off, and a ballot names the rows that have a band entry in the strip.
// Those rows in ascending order, and in each the set bits f in ascending
// order: the whole wave computes dot(r[b, :], W[64 s + f, :]), lanes striding
// over d (float4 where `vec` says that every row is 16-byte aligned, scalar
// otherwise) and one xor tree, after which every lane holds the sum.  Lane f
// owns feature f: it alone adds (gscale inv[j]) dot to its accumulator and 1
// to its count.  So the order of a feature's sum within a wave is the rows
// ascending, and the waves' partials are added per feature in wave order
// through LDS by wave 0, which stores
//   g_theta[m, j] = 0 - (theta[j] sum + l0_alpha count / B) / eps
// with a plain store: an empty band gives +0.
// ---------------------------------------------------------------------------
SPK_DEV float jgt_dot(const float* __restrict__ rrow, const float* __restrict__ wrow, int d, int lane,
                      bool vec) {
  float acc = 0.f;
  if (vec) {
    const spk_f32x4* __restrict__ r4 = (const spk_f32x4*)rrow;
    const spk_f32x4* __restrict__ w4 = (const spk_f32x4*)wrow;
    const int d4 = d >> 2;
#pragma unroll 2
    for (int i = lane; i < d4; i += WAVE) {
      const spk_f32x4 a = r4[i], w = w4[i];
      acc = __builtin_fmaf(a.x, w.x, acc);
      acc = __builtin_fmaf(a.y, w.y, acc);
      acc = __builtin_fmaf(a.z, w.z, acc);
      acc = __builtin_fmaf(a.w, w.w, acc);
    }
  } else {
#pragma unroll 4
    for (int i = lane; i < d; i += WAVE) acc = __builtin_fmaf(rrow[i], wrow[i], acc);
  }
  return spk_wave_sum(acc, lane);
}

__global__ __launch_bounds__(JGT_T) SPK_NOPK
void k_jump_grad_theta(const unsigned long long* __restrict__ band_bits,  // [M, B, NW]
                       const float* __restrict__ Wdec,       // [M, n, d]
                       const float* __restrict__ inv_norms,  // [M, n]
                       const float* __restrict__ r,          // [M, B, d]
                       const float* __restrict__ threshold,  // [M, n]
                       const float* __restrict__ bandwidth,  // [M]
                       const float* __restrict__ l0_alpha,   // [M]
                       float* __restrict__ g_theta,          // [M, n]
                       int B, int d, int n, int NW, int vec) {
  __shared__ float part[JGT_NW][JGT_STRIP];
  __shared__ int cntp[JGT_NW][JGT_STRIP];
  const int lane = spk_tid() & (WAVE - 1);
  const int wave = spk_wave_id();
  const int m = (int)__builtin_amdgcn_workgroup_id_y();
  const int strip = (int)__builtin_amdgcn_workgroup_id_x();
  const int j0 = strip * JGT_STRIP;
  const int left = n - j0;  // >= 1: the grid has NW = ceil(n / 64) strips
  const unsigned long long valid = left >= WAVE ? ~0ull : ((1ull << left) - 1ull);
  const int jl = j0 + spk_min(lane, left - 1);  // the lane's feature, held inside n

  const unsigned long long* words = band_bits + (long)m * B * NW + strip;
  const float* W = Wdec + ((long)m * n + j0) * d;
  const float* r_m = r + (long)m * B * d;
  const float scale = (2.0f / ((float)B * (float)d)) * inv_norms[(long)m * n + jl];

  float acc = 0.f;
  int cnt = 0;
  for (int i0 = 0; i0 * JGT_NW + wave < B; i0 += WAVE) {
    const int bl = (i0 + lane) * JGT_NW + wave;  // the lane's row of this round
    unsigned long long word = bl < B ? words[(long)bl * NW] & valid : 0ull;
    const int lo = (int)(unsigned)word, hi = (int)(unsigned)(word >> 32);
    unsigned long long rows = spk_ballot(word != 0ull);
    while (rows) {
      const int L = __builtin_ctzll(rows);
      rows &= rows - 1;
      const int b = (i0 + L) * JGT_NW + wave;
      unsigned long long bits = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(hi, L) << 32) |
                                (unsigned long long)(unsigned)__builtin_amdgcn_readlane(lo, L);
      const float* rrow = r_m + (long)b * d;
      while (bits) {
        const int f = __builtin_ctzll(bits);
        bits &= bits - 1;
        const float dot = jgt_dot(rrow, W + (long)f * d, d, lane, vec != 0);
        if (lane == f) {
          acc += scale * dot;
          cnt += 1;
        }
      }
    }
  }
  part[wave][lane] = acc;
  cntp[wave][lane] = cnt;
  spk_barrier();
  if (wave == 0 && lane < left) {
    float s = part[0][lane];
    int k = cntp[0][lane];
#pragma unroll
    for (int w = 1; w < JGT_NW; ++w) {
      s += part[w][lane];
      k += cntp[w][lane];
    }
    const float th = threshold[(long)m * n + j0 + lane];
    g_theta[(long)m * n + j0 + lane] = 0.f - (th * s + l0_alpha[m] * (float)k / (float)B) / bandwidth[m];
  }
}
