// The uncompressed COCO run-length code back into bit words (fs_rle_bits: fs_mask_rle's inverse; no counterpart in the reference:
// UNPINNED, the format restated from its published definition).  All of it is integer work; every word of the result
// is written by a plain store, nothing is zeroed beforehand and nothing is read on the host.
//   The code lists run lengths of 0, 1, 0, ... over the mask flattened column-major, p = x * Hs + y.  With end[r] = the sum of the
//   first r + 1 counts, pixel p belongs to run r(p) = the first r with end[r] > p, and its value is r(p) & 1: zero-length runs repeat
//   an end and are stepped over, so every well-formed code decodes, canonical or not.
//   scan   one workgroup an image: the inclusive int64 sum of the n_read = min(max(n_runs, 0), cap) counts, tile after tile of 256,
//          each end clamped to 0 .. N and kept as an int in scratch; the same sweep sees a negative count and sums the odd-indexed
//          counts; one lane writes the info row and the image's (status, n_read) behind the ends.
//   words  a wave owns 64 adjacent columns and 64 rows, lane <-> column.  A lane finds the run of its first pixel by bisection and
//          walks down its column, stepping the run index while end[r] <= p; a ballot over the wave is a row's two words.  Lane i
//          keeps the ballot of row i, and the 64 rows are stored at once.  A column is a contiguous stretch of positions, so a lane's
//          reads of end[] are a contiguous stretch too, next to its neighbours'.  An image whose status is not 0 stores zeros.
// Every index into counts, scratch, info and bits is bounded by B, Hs, Ws, cap and n_read alone: the ends are compared, never used
// as addresses.
#include "mask_words.h"

namespace {

constexpr int DEC_THREADS = 256;
constexpr int DEC_WAVES = DEC_THREADS / 64;
constexpr int DEC_ROWS = 64;                           // rows a wave: one kept ballot a lane
enum { DEC_OK = 0, DEC_CUT = 1, DEC_BAD = 2, DEC_SUM = 3 };

struct DecodePlan {
  long P, tiles_x, tiles_y, per;                       // words a row; 64-column groups; 256-row groups; workgroups an image
  long ends, meta, total;                              // scratch, in ints: end[B][cap], then (status, n_read)[B]
  bool ok;
};

DecodePlan decode_plan(int B, int Hs, int Ws, int cap) {
  DecodePlan p = {};
  if (!(B > 0 && cap > 0)) return p;
  p.ends = 0, p.meta = (long)B * cap, p.total = p.meta + 2L * B;
  if (!(Hs > 0 && Ws > 0 && (long)Hs * Ws < MASK_INT_LIMIT)) return p;
  p.P = mask_row_words(Ws);
  p.tiles_x = cdiv(Ws, 64), p.tiles_y = cdiv(Hs, DEC_ROWS * DEC_WAVES), p.per = p.tiles_x * p.tiles_y;
  // a workgroup covers at most 2^14 bit slots of its own, so the grid stays below 2^31 with the slots below 2^32
  p.ok = (long)B * Hs * p.P * 32 <= THREADS_MAX && (long)B * p.per < MASK_INT_LIMIT;
  return p;
}

__device__ __forceinline__ long long dec_wave_scan(long long v, int lane) {           // inclusive, over the wave
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const long long u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  return v;
}

// grid = B.  end[b][i] = clamp(counts[b][0] + ... + counts[b][i], 0, N), i < n_read; info[b] = (status, area, n_read, total)
__global__ __launch_bounds__(DEC_THREADS) void rle_decode_scan_kernel(const int* __restrict__ counts, const long long* __restrict__ n_runs,
                                                                      int n_stride, long long* __restrict__ info, int* __restrict__ ends,
                                                                      int* __restrict__ meta, int N, int cap) {
  __shared__ long long wsum[DEC_WAVES];
  __shared__ long long osum[DEC_WAVES];
  __shared__ int wneg[DEC_WAVES];
  const size_t b = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long n = n_runs[b * (size_t)n_stride];
  const int n_read = (int)(n < 0 ? 0 : (n > cap ? (long long)cap : n));
  const int* c = counts + b * (size_t)cap;
  int* e = ends + b * (size_t)cap;
  long long carry = 0, odd = 0;
  int neg = 0;
  for (int base = 0; base < n_read; base += DEC_THREADS) {                           // uniform: base and n_read are the workgroup's
    const int i = base + (int)threadIdx.x;
    const int v = i < n_read ? c[i] : 0;
    neg |= v < 0;
    if (i & 1) odd += v;
    long long s = dec_wave_scan((long long)v, lane);
    if (lane == 63) wsum[wave] = s;
    __syncthreads();
    long long before = carry, all = carry;
#pragma unroll
    for (int w = 0; w < DEC_WAVES; ++w) {
      if (w < wave) before += wsum[w];
      all += wsum[w];
    }
    s += before;
    if (i < n_read) e[i] = (int)(s < 0 ? 0 : (s > N ? (long long)N : s));
    carry = all;
    __syncthreads();
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    odd += __shfl_xor(odd, o, 64);
    neg |= __shfl_xor(neg, o, 64);
  }
  if (lane == 0) osum[wave] = odd, wneg[wave] = neg;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long area = 0;
    int bad = 0;
    for (int w = 0; w < DEC_WAVES; ++w) area += osum[w], bad |= wneg[w];
    const int status = n > cap ? DEC_CUT : (n < 1 || bad) ? DEC_BAD : carry != (long long)N ? DEC_SUM : DEC_OK;
    info[b * 4 + 0] = status;
    info[b * 4 + 1] = status == DEC_OK ? area : 0;
    info[b * 4 + 2] = n_read;
    info[b * 4 + 3] = carry;
    meta[b * 2 + 0] = status;
    meta[b * 2 + 1] = n_read;
  }
}

// grid = B * tiles_x * tiles_y; wave w of workgroup (tx, ty) takes columns 64 tx .. and rows 256 ty + 64 w ..
__global__ __launch_bounds__(DEC_THREADS) void rle_decode_words_kernel(const int* __restrict__ ends, const int* __restrict__ meta,
                                                                       unsigned int* __restrict__ bits, int Hs, int Ws, int P, int cap,
                                                                       int tiles_x, int per) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int img = blockIdx.x / per, t = blockIdx.x - img * per;
  const int ty = t / tiles_x, tx = t - ty * tiles_x;
  const int y0 = ty * (DEC_ROWS * DEC_WAVES) + wave * DEC_ROWS;
  if (y0 >= Hs) return;                                // the wave's, not a lane's: no barrier below
  const int y1 = min(y0 + DEC_ROWS, Hs);
  const int x = tx * 64 + lane;
  const int status = meta[(size_t)img * 2], n_read = meta[(size_t)img * 2 + 1];
  const int* e = ends + (size_t)img * cap;
  unsigned long long keep = 0ull;
  if (status == DEC_OK) {                              // n_read >= 1 and end[n_read - 1] = N > every position
    const bool live = x < Ws;
    int p = live ? x * Hs + y0 : 0;                    // below N < 2^31
    int r = 0, er = 0;
    if (live) {
      int lo = 0, hi = n_read - 1;                     // the first r with end[r] > p
      while (lo < hi) {
        const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
        if (e[mid] > p) hi = mid; else lo = mid + 1;
      }
      r = lo, er = e[r];
    }
    for (int y = y0; y < y1; ++y, ++p) {
      if (live) {
        while (er <= p && r < n_read - 1) er = e[++r];
      }
      const unsigned long long row = __ballot(live && (r & 1));
      if (lane == y - y0) keep = row;
    }
  }
  const int y = y0 + lane;
  if (y < y1) {
    unsigned int* dst = bits + ((size_t)img * Hs + y) * P + 2 * tx;
    dst[0] = (unsigned int)keep;
    if (2 * tx + 1 < P) dst[1] = (unsigned int)(keep >> 32);
  }
}

}  // namespace

extern "C" {

long fs_rle_bits_scratch_ints(int B, int cap) { return decode_plan(B, 1, 1, cap).total; }

int fs_rle_bits(const int* counts, const long long* n_runs, int n_stride, unsigned int* bits, long long* info, int* scratch, int B, int Hs,
                int Ws, int cap, hipStream_t stream) {
  const DecodePlan p = decode_plan(B, Hs, Ws, cap);
  FS_REQUIRE(counts && n_runs && bits && info && scratch && n_stride >= 1 && p.ok);
  int* ends = scratch + p.ends;
  int* meta = scratch + p.meta;
  hipLaunchKernelGGL(rle_decode_scan_kernel, dim3((unsigned)B), dim3(DEC_THREADS), 0, stream, counts, n_runs, n_stride, info, ends, meta,
                     Hs * Ws, cap);
  FS_LAUNCH_CHECK();
  hipLaunchKernelGGL(rle_decode_words_kernel, dim3((unsigned)((long)B * p.per)), dim3(DEC_THREADS), 0, stream, (const int*)ends,
                     (const int*)meta, bits, Hs, Ws, (int)p.P, cap, (int)p.tiles_x, (int)p.per);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

}  // extern "C"
