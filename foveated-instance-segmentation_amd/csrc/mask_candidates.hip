// Of an image's annotated instances, the one under the gaze (fs_mask_candidates).  The reference builds its labels by choosing one
// annotation and putting the gaze on a pixel inside it (DynamicFocus/e_preprocess_scripts/b2_preprocess_lvis.py:258-333: rasterise the
// annotation, ridx_rrcc = np.random.randint(len(rrs))); this is the inverse of that step -- gaze and annotations given, which one is
// looked at -- and has no counterpart there.  UNPINNED: the definition is this library's (include/fovealseg.h).  All
// of it is integer work on bit words (mask_words.h: the layout), by plain stores, without atomics and without a host read.  Passes:
//   valid   one workgroup: cand_off[0] == 0, non-decreasing, cand_off[B] == N -> scratch[0].  Decided once; every later pass reads it.
//   count   the hot pass, one workgroup per (candidate, band of rows): the candidate finds its image by bisecting cand_off (positions
//           only: no offset value forms an address), then reads its words once -- four a 16-byte load where a row is whole groups of
//           four and the planes are 16-byte aligned -- and the image's prediction words beside them (re-read by every candidate of the
//           image: L2).  Per word the popcounts |c|, |c & p|, |p| and the nearest set pixel to the gaze as mask_near_key.  Shuffles
//           in the wave, LDS across the waves, one lane stores the band's record (area, inter, parea, key) into scratch.
//   select  a wave per image: each lane adds the band records of its candidates in index order, writes their cand rows and keeps the
//           least (d2, area, n) and the greatest IoU with the prediction (cross-multiplied in int64); shuffles, then one lane writes sel.
//   copy    one workgroup per (image, band of rows): the selected candidate's words with the tail masked, or zeros, into gbits.
// Sums and minima of integers in a fixed order, and total orders with the row as the last key: the same bits in every run.
#include "mask_words.h"

namespace {

constexpr int CAND_THREADS = 256;
constexpr int CAND_WAVES = CAND_THREADS / 64;
constexpr int CAND_BAND_ROWS = 256;                    // the count pass: rows a band at the most
constexpr int CAND_BAND_WORDS = 8192;                  // ... and words a band at the most (one row where a row is longer): 32 a thread
constexpr int CAND_COPY_ROWS = 64;                     // the copy pass: it has B images to fill the machine with, not N candidates
constexpr int CAND_COPY_WORDS = 2048;
constexpr int CAND_REC = 5;                            // ints a (candidate, band) record: area, inter, parea, key low, key high
constexpr int CAND_HEAD = 4;                           // ints in front of the records: [0] = 1 where cand_off is malformed

struct CandPlan {
  int P, rows, bands;                                  // words a row; the count pass: rows a band, bands an image
  int crows, cbands;                                   // the copy pass: rows a band, bands an image
  bool vec;                                            // rows are whole 16-byte groups: the count pass may read four words a load
  long scratch;                                        // in ints
  bool ok;
};

CandPlan cand_plan(int B, int N, int Hs, int Ws) {
  CandPlan p = {};
  // sides: d2 < 2^29, key < 2^60, inter * union < 2^57; pixel indices are ints, and the key keeps them in 31 bits
  if (!(B > 0 && N >= 0 && Hs > 0 && Ws > 0 && Hs <= MASK_MAX_SIDE && Ws <= MASK_MAX_SIDE && (long)Hs * Ws < MASK_INT_LIMIT)) return p;
  p.P = mask_row_words(Ws);
  // Measured on one MI355X at B = 64, 1024^2, 64 candidates an image (profiles/r31/README.md): bands of 64 rows / 2048 words 190 us a
  // call, 256 rows / 8192 words 147 us (the count pass 167 -> 121 us, the copy pass 7.6 -> 16.5 us: hence its own, smaller bands),
  // 16 rows / 512 words 442 us; one word a load instead of four 268 and 230 us.  FS_CAND_ROWS / FS_CAND_WORDS / FS_CAND_VEC exist in
  // kernel A/B builds only.
  static const int band_rows = FS_ENV_INT("FS_CAND_ROWS", CAND_BAND_ROWS), band_words = FS_ENV_INT("FS_CAND_WORDS", CAND_BAND_WORDS);
  static const int vec = FS_ENV_INT("FS_CAND_VEC", 4);
  const int fit = max(1, band_words / p.P);            // >= 4: P <= 512
  p.rows = min(Hs, min(band_rows, fit));
  p.vec = vec == 4 && p.P % 4 == 0;
  p.bands = cdiv(Hs, p.rows);
  p.crows = min(Hs, min(CAND_COPY_ROWS, max(1, CAND_COPY_WORDS / p.P)));
  p.cbands = cdiv(Hs, p.crows);
  p.scratch = CAND_HEAD + (long)N * p.bands * CAND_REC;
  p.ok = (long)N * p.bands <= MASK_INT_LIMIT && (long)B * p.cbands <= MASK_INT_LIMIT;     // the grids of the count and copy passes
  return p;
}

// head[0] = 1 unless cand_off[0] == 0 <= cand_off[1] <= ... <= cand_off[B] == N; one workgroup
__global__ __launch_bounds__(CAND_THREADS) void cand_valid_kernel(const int* __restrict__ cand_off, int* __restrict__ head, int B, int N) {
  int bad = 0;
  for (int i = threadIdx.x; i < B; i += CAND_THREADS) bad |= cand_off[i] > cand_off[i + 1];
  if (threadIdx.x == 0) bad |= cand_off[0] != 0 || cand_off[B] != N;
  bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) head[0] = bad ? 1 : 0;
}

// grid = N * bands.  rec[n, band] = (|c|, |c & p|, |p|, key) over the band's rows; with malformed offsets only |c| is formed.
// VEC = 4 reads four words of a row by one 16-byte load a lane (P % 4 == 0 and 16-byte aligned planes), VEC = 1 one word.
template <int VEC>
__global__ __launch_bounds__(CAND_THREADS) void cand_count_kernel(const unsigned int* __restrict__ cbits, const int* __restrict__ cand_off,
                                                                  const float* __restrict__ focus, const unsigned int* __restrict__ pbits,
                                                                  int* __restrict__ scratch, int B, int Hs, int Ws, int P, int rows, int bands) {
  __shared__ unsigned long long red_k[CAND_WAVES];
  __shared__ int red_c[CAND_WAVES][3];
  const int tid = threadIdx.x;
  const int n = blockIdx.x / bands, band = blockIdx.x - n * bands;
  const int PV = P / VEC;                              // loads a row
  const int r0 = band * rows, items = min(rows, Hs - r0) * PV;
  const bool bad = scratch[0] != 0;
  int b = 0;
  if (!bad) {                                          // the last b with cand_off[b] <= n: cand_off[0] = 0 <= n < N = cand_off[B]
    int lo = 0, hi = B;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (cand_off[mid] <= n) lo = mid;
      else hi = mid;
    }
    b = lo;
  }
  const unsigned int* cw = cbits + ((size_t)n * Hs + r0) * P;
  const unsigned int* pw = (pbits && !bad) ? pbits + ((size_t)b * Hs + r0) * P : nullptr;
  int py = 0, px = 0;
  if (!bad) py = mask_gaze_px(mask_gaze16(focus[2 * (size_t)b], Hs)), px = mask_gaze_px(mask_gaze16(focus[2 * (size_t)b + 1], Ws));
  // a thread's loads are CAND_THREADS apart: (row, column) move by a fixed step, one division a thread
  const int qs = CAND_THREADS / PV, rs = CAND_THREADS - qs * PV;
  int y = r0 + tid / PV, cv = tid - (tid / PV) * PV;
  unsigned long long key = ~0ull;
  int area = 0, inter = 0, parea = 0;                  // at most 8192 * 32 a band
  for (int i = tid; i < items; i += CAND_THREADS) {
    unsigned int mw[VEC], pv[VEC];
    if constexpr (VEC == 4) {
      const uint4 v = reinterpret_cast<const uint4*>(cw)[i];
      mw[0] = v.x, mw[1] = v.y, mw[2] = v.z, mw[3] = v.w;
      const uint4 q = pw ? reinterpret_cast<const uint4*>(pw)[i] : make_uint4(0u, 0u, 0u, 0u);
      pv[0] = q.x, pv[1] = q.y, pv[2] = q.z, pv[3] = q.w;
    } else {
      mw[0] = cw[i];
      pv[0] = pw ? pw[i] : 0u;
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const int c = cv * VEC + j;
      const unsigned int tail = mask_tail(c, P, Ws);
      const unsigned int m = mw[j] & tail, p = pv[j] & tail;
      inter += __popc(m & p);
      parea += __popc(p);
      if (m == 0u) continue;
      area += __popc(m);
      if (bad) continue;
      key = mask_near_key(key, m, y, c, py, px, Ws);
    }
    y += qs, cv += rs;
    if (cv >= PV) cv -= PV, ++y;
  }
  key = mask_key_wave_min(key);
  area = wave_sum_i(area), inter = wave_sum_i(inter), parea = wave_sum_i(parea);
  if ((tid & 63) == 0) red_k[tid >> 6] = key, red_c[tid >> 6][0] = area, red_c[tid >> 6][1] = inter, red_c[tid >> 6][2] = parea;
  __syncthreads();
  if (tid != 0) return;
  for (int w = 1; w < CAND_WAVES; ++w) {
    key = red_k[w] < key ? red_k[w] : key;
    area += red_c[w][0], inter += red_c[w][1], parea += red_c[w][2];
  }
  int* r = scratch + CAND_HEAD + (size_t)blockIdx.x * CAND_REC;
  r[0] = area, r[1] = inter, r[2] = parea, r[3] = (int)(unsigned int)(key & 0xffffffffull), r[4] = (int)(unsigned int)(key >> 32);
}

struct CandPick {                                      // the selected instance so far: the least (k = d2 * 2^31 + area, n); n = -1: none
  unsigned long long k;
  long long inter;
  int n;
};
struct CandBest {                                      // the best-overlapping instance so far; n = -1: none
  long long inter, uni, area;
  int n;
};

__device__ __forceinline__ bool cand_pick_before(const CandPick& a, const CandPick& b) {       // a goes before b
  if (a.n < 0 || b.n < 0) return b.n < 0 && a.n >= 0;
  return a.k < b.k || (a.k == b.k && a.n < b.n);
}
__device__ __forceinline__ bool cand_best_before(const CandBest& a, const CandBest& b) {
  if (a.n < 0 || b.n < 0) return b.n < 0 && a.n >= 0;
  const long long l = a.inter * b.uni, r = b.inter * a.uni;                                    // a.inter / a.uni against b.inter / b.uni, below 2^57
  if (l != r) return l > r;
  if (a.area != b.area) return a.area < b.area;
  return a.n < b.n;
}

// grid = B, one wave.  cand rows of the image's candidates, and sel[b]; with malformed offsets the images share out all N rows.
__global__ __launch_bounds__(64) void cand_select_kernel(const int* __restrict__ cand_off, const long long* __restrict__ cand_cat,
                                                         const int* __restrict__ scratch, long long* __restrict__ cand,
                                                         long long* __restrict__ sel, int B, int N, int Ws, int bands, long long snap2) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int* recs = scratch + CAND_HEAD;
  long long* s = sel + (size_t)b * 8;
  if (scratch[0] != 0) {
    for (long n = (long)b * 64 + lane; n < N; n += (long)B * 64) {
      long long area = 0;
      for (int i = 0; i < bands; ++i) area += recs[((size_t)n * bands + i) * CAND_REC];
      long long* o = cand + (size_t)n * 6;
      o[0] = -1, o[1] = area, o[2] = 0, o[3] = -1, o[4] = -1, o[5] = -1;
    }
    if (lane == 0) s[0] = -1, s[1] = -1, s[2] = -1, s[3] = 0, s[4] = 0, s[5] = 0, s[6] = -1, s[7] = 1;
    return;
  }
  const int lo = cand_off[b], hi = cand_off[b + 1];    // valid: 0 <= lo <= hi <= N
  long long parea = 0;                                 // |p_b|: every candidate's records carry it, the first one's are read
  if (lo < hi)
    for (int i = 0; i < bands; ++i) parea += recs[((size_t)lo * bands + i) * CAND_REC + 2];
  CandPick pick = {0ull, 0, -1};
  CandBest best = {0, 1, 0, -1};
  int hits = 0;
  for (int n = lo + lane; n < hi; n += 64) {
    long long area = 0, inter = 0;
    unsigned long long key = ~0ull;
    for (int i = 0; i < bands; ++i) {                  // in index order
      const int* r = recs + ((size_t)n * bands + i) * CAND_REC;
      area += r[0], inter += r[1];
      const unsigned long long k = (unsigned long long)(unsigned int)r[3] | ((unsigned long long)(unsigned int)r[4] << 32);
      key = k < key ? k : key;
    }
    long long d2 = -1, ny = -1, nx = -1;
    if (area > 0) {
      const long long at = (long long)(key & 0x7fffffffull);
      d2 = (long long)(key >> 31), ny = at / Ws, nx = at - ny * Ws;
    }
    long long* o = cand + (size_t)n * 6;
    o[0] = b, o[1] = area, o[2] = inter, o[3] = d2, o[4] = ny, o[5] = nx;
    if (area > 0) {
      hits += d2 == 0;
      if (d2 <= snap2) {
        const CandPick mine = {((unsigned long long)d2 << 31) | (unsigned long long)area, inter, n};
        if (cand_pick_before(mine, pick)) pick = mine;
      }
      if (inter > 0) {
        const CandBest mine = {inter, area + parea - inter, area, n};
        if (cand_best_before(mine, best)) best = mine;
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const CandPick p = {__shfl_xor(pick.k, o, 64), __shfl_xor(pick.inter, o, 64), __shfl_xor(pick.n, o, 64)};
    if (cand_pick_before(p, pick)) pick = p;
    const CandBest q = {__shfl_xor(best.inter, o, 64), __shfl_xor(best.uni, o, 64), __shfl_xor(best.area, o, 64), __shfl_xor(best.n, o, 64)};
    if (cand_best_before(q, best)) best = q;
    hits += __shfl_xor(hits, o, 64);
  }
  if (lane != 0) return;
  const bool any = pick.n >= 0;
  s[0] = pick.n;
  s[1] = (any && cand_cat) ? cand_cat[pick.n] : -1;    // the only read of cand_cat: at a selected row
  s[2] = any ? (long long)(pick.k >> 31) : -1;
  s[3] = any ? (long long)(pick.k & 0x7fffffffull) : 0;
  s[4] = any ? pick.inter : 0;
  s[5] = hits, s[6] = best.n, s[7] = 0;
}

// grid = B * bands: gbits[b]'s band = the selected candidate's words within x < Ws, or zeros
__global__ __launch_bounds__(CAND_THREADS) void cand_copy_kernel(const unsigned int* __restrict__ cbits, const long long* __restrict__ sel,
                                                                 unsigned int* __restrict__ gbits, int Hs, int Ws, int P, int rows, int bands) {
  const int tid = threadIdx.x;
  const int b = blockIdx.x / bands, band = blockIdx.x - b * bands;
  const int r0 = band * rows, nw = min(rows, Hs - r0) * P;
  const long long at = sel[(size_t)b * 8];
  unsigned int* dst = gbits + ((size_t)b * Hs + r0) * P;
  if (at < 0) {                                        // uniform over the workgroup
    for (int i = tid; i < nw; i += CAND_THREADS) dst[i] = 0u;
    return;
  }
  const unsigned int* src = cbits + ((size_t)at * Hs + r0) * P;
  const int rs = CAND_THREADS % P;
  int c = tid % P;
  for (int i = tid; i < nw; i += CAND_THREADS) {
    dst[i] = src[i] & mask_tail(c, P, Ws);
    c += rs;
    if (c >= P) c -= P;
  }
}

}  // namespace

extern "C" {

long fs_mask_candidates_scratch_ints(int B, int N, int Hs, int Ws) {
  const CandPlan p = cand_plan(B, N, Hs, Ws);
  return p.ok ? p.scratch : 0;
}

int fs_mask_candidates(const unsigned int* cbits, const int* cand_off, const long long* cand_cat, const float* focus,
                       const unsigned int* pbits, long long* cand, long long* sel, unsigned int* gbits, int* scratch, int B, int N, int Hs,
                       int Ws, long snap2, hipStream_t stream) {
  const CandPlan p = cand_plan(B, N, Hs, Ws);
  FS_REQUIRE(p.ok && (N == 0 || (cbits && cand)) && cand_off && focus && sel && gbits && scratch && snap2 >= 0 && gbits != cbits);
  hipLaunchKernelGGL(cand_valid_kernel, dim3(1), dim3(CAND_THREADS), 0, stream, cand_off, scratch, B, N);
  FS_LAUNCH_CHECK();
  if (N > 0) {
    // 16-byte loads want 16-byte aligned planes: with P % 4 == 0 every row of an aligned tensor is
    const bool vec = p.vec && (reinterpret_cast<uintptr_t>(cbits) & 15) == 0 && (reinterpret_cast<uintptr_t>(pbits) & 15) == 0;
    hipLaunchKernelGGL(vec ? cand_count_kernel<4> : cand_count_kernel<1>, dim3((unsigned)((long)N * p.bands)), dim3(CAND_THREADS), 0, stream,
                       cbits, cand_off, focus, pbits, scratch, B, Hs, Ws, p.P, p.rows, p.bands);
    FS_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(cand_select_kernel, dim3((unsigned)B), dim3(64), 0, stream, cand_off, cand_cat, (const int*)scratch, cand, sel, B, N, Ws,
                     p.bands, (long long)snap2);
  FS_LAUNCH_CHECK();
  hipLaunchKernelGGL(cand_copy_kernel, dim3((unsigned)((long)B * p.cbands)), dim3(CAND_THREADS), 0, stream, cbits, (const long long*)sel, gbits,
                     Hs, Ws, p.P, p.crows, p.cbands);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

}  // extern "C"
