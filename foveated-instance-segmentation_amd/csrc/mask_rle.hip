// Bit words from a byte mask, and their statistics and uncompressed COCO run-length code (fs_mask_bits, fs_mask_rle; mask_words.h: the
// layout).  The code reads the mask column-major (p = x * Hs + y) and lists the distances between the boundaries
// T = {p : v[p] != v[p-1]}, v[-1] = 0 (format restated from its published definition; unpinned).
//   bits     one lane a column, a ballot a word: the byte mask's "non-zero" packed (mask_bits_kernel); the un-warp gather packs its own
//            words the same way (unwarp.hip: gather_bits)
//   count    one thread per (column, RLE_SEG-row segment): the boundaries in it, the position of its last one, its set pixels and
//            their row range (rle_walk_kernel<false>)
//   scan     one workgroup per image over its items in column-major order, which is the order of the runs: the exclusive sum of the
//            boundary counts = where an item's first count goes, the running maximum of the last positions = the boundary before it;
//            the same sweep sums the area, takes the box, and writes stats and the closing count (rle_scan_kernel)
//   store    the walk again, storing counts[offset + i] = boundary - the one before, below cap (rle_walk_kernel<true>)
// Plain stores only: the same bits in any order.  counts is zeroed by the launcher, so everything past the code reads 0.
#include "mask_words.h"

namespace {

constexpr int RLE_SEG = 64;                            // rows per item: 16 items a column at 1024 rows

// the same words from a byte mask (non-zero = set), any alignment
__global__ __launch_bounds__(256) void mask_bits_kernel(const unsigned char* __restrict__ mask, unsigned int* __restrict__ bits, int Ws, int P,
                                                        long words) {
  const BitSlot sl = bit_slot<32>(Ws, P, words);
  store_word_ballot(bits, sl.g, words, sl.live && mask[sl.row * Ws + sl.x] != 0);
}
// Item (x, s) = rows s * RLE_SEG .. of column x, item index x * S + s: column-major.  Lanes take neighbouring columns of one segment, so a
// wave reads two words a row.  The pixel above the top of column x > 0 is the bottom of column x - 1; above pixel (0,0) it is 0.
// STORE = false: cnt[item] = boundaries in the item, last[item] = position of its last one (0 without: no boundary lies before
// position 0, and positions only grow along the items), st[item] = set pixels | (first set row in the segment) << 8 | (last) << 16.
// STORE = true: cnt / last hold the scan's results (see rle_scan_kernel), and the item's i-th boundary at position p stores
// counts[cnt + i] = p - the boundary before it, where cnt + i < cap.
template <bool STORE>
__global__ __launch_bounds__(256) void rle_walk_kernel(const unsigned int* __restrict__ bits, int* __restrict__ cnt, int* __restrict__ last,
                                                       int* __restrict__ st, int* __restrict__ counts, int Hs, int Ws, int P, int S,
                                                       int blocks_per_image, int cap) {
  const int b = blockIdx.x / blocks_per_image;
  const int g = (blockIdx.x - b * blocks_per_image) * 256 + (int)threadIdx.x;
  const int M = Ws * S;
  if (g >= M) return;
  const int s = g / Ws, x = g - s * Ws;
  const long item = (long)b * M + (long)x * S + s;
  const unsigned int* ib = bits + (long)b * Hs * P;
  const unsigned int* col = ib + (x >> 5);
  const int y0 = s * RLE_SEG, y1 = min(y0 + RLE_SEG, Hs);
  unsigned int prev = 0u;
  if (s > 0) prev = mask_bit(col[(long)(y0 - 1) * P], x);
  else if (x > 0) prev = mask_bit(ib[(long)(Hs - 1) * P + ((x - 1) >> 5)], x - 1);
  int n = 0, pos = 0, area = 0, ylo = 0, yhi = 0;
  int* out = nullptr;
  if (STORE) { n = cnt[item]; pos = last[item]; out = counts + (long)b * cap; }
  const int p0 = x * Hs;
  for (int y = y0; y < y1; ++y) {
    const unsigned int v = mask_bit(col[(long)y * P], x);
    if (v != prev) {
      if (STORE) {
        if (n < cap) out[n] = p0 + y - pos;
      }
      pos = p0 + y;
      ++n;
    }
    if (!STORE && v) {
      if (area == 0) ylo = y - y0;
      yhi = y - y0;
      ++area;
    }
    prev = v;
  }
  if (!STORE) { cnt[item] = n; last[item] = pos; st[item] = area | ylo << 8 | yhi << 16; }
}
// One workgroup per image; thread t owns the items [t * chunk, (t+1) * chunk) of its M = Ws * S.  cnt[item] <- the boundaries before the
// item, last[item] <- the position of the last boundary before it (0 = none: the code's first count is T[0] - 0).  stats[b] = (area,
// x0, y0, bw, bh, n_runs) and counts[b, n_runs - 1] = N - the last boundary, where it lies below cap.
__global__ __launch_bounds__(256) void rle_scan_kernel(int* __restrict__ cnt, int* __restrict__ last, const int* __restrict__ st,
                                                       long long* __restrict__ stats, int* __restrict__ counts, int Hs, int Ws, int S, int cap) {
  __shared__ int psum[256], pmax[256];
  __shared__ long long red[16];
  __shared__ int box[4];                               // max of: Ws - x, x + 1, Hs - y, y + 1 over the set pixels; 0 = none
  const int b = blockIdx.x, tid = threadIdx.x;
  const int M = Ws * S;
  int* c = cnt + (long)b * M;
  int* l = last + (long)b * M;
  const int* sp = st + (long)b * M;
  const int chunk = (M + 255) / 256;
  const int i0 = min(tid * chunk, M), i1 = min(i0 + chunk, M);
  if (tid < 4) box[tid] = 0;
  int sum = 0, mx = 0, bx[4] = {0, 0, 0, 0};
  long long area = 0;
  for (int i = i0; i < i1; ++i) {
    sum += c[i];
    mx = max(mx, l[i]);
    const int w = sp[i], a = w & 255;
    if (a) {
      const int x = i / S, yb = (i - x * S) * RLE_SEG;
      area += a;
      bx[0] = max(bx[0], Ws - x); bx[1] = max(bx[1], x + 1);
      bx[2] = max(bx[2], Hs - (yb + ((w >> 8) & 255))); bx[3] = max(bx[3], yb + ((w >> 16) & 255) + 1);
    }
  }
  psum[tid] = sum; pmax[tid] = mx;
  __syncthreads();
  if (area) {
#pragma unroll
    for (int q = 0; q < 4; ++q) atomicMax(&box[q], bx[q]);
  }
  if (tid == 0) {                                      // exclusive sum and exclusive running maximum over the 256 chunks
    int cs = 0, cm = 0;
    for (int t = 0; t < 256; ++t) {
      const int vs = psum[t], vm = pmax[t];
      psum[t] = cs; pmax[t] = cm;
      cs += vs; cm = max(cm, vm);
    }
  }
  __syncthreads();
  int run = psum[tid], pm = pmax[tid];
  for (int i = i0; i < i1; ++i) {
    const int n = c[i], p = l[i];
    c[i] = run; l[i] = pm;
    run += n; pm = max(pm, p);
  }
  area = block_sum<long long>(area, red);
  if (tid == 255) {                                    // its run / pm have passed every item: |T| and T[last]
    long long* o = stats + (long)b * 6;
    const bool any = area != 0;
    o[0] = area;
    o[1] = any ? Ws - box[0] : 0; o[2] = any ? Hs - box[2] : 0;
    o[3] = any ? box[1] - (Ws - box[0]) : 0; o[4] = any ? box[3] - (Hs - box[2]) : 0;
    o[5] = (long long)run + 1;
    if (run < cap) counts[(long)b * cap + run] = Hs * Ws - pm;
  }
}

}  // namespace

RlePlan rle_plan(int B, int Hs, int Ws) {
  RlePlan r = {};
  if (!(B > 0 && Hs > 0 && Ws > 0)) return r;
  r.P = mask_row_words(Ws), r.words = (long)B * Hs * r.P;
  r.S = cdiv(Hs, RLE_SEG), r.M = (long)Ws * r.S, r.bpi = cdiv(r.M, 256);
  r.cnt = 0, r.last = (long)B * r.M, r.st = 2 * r.last, r.total = 3 * r.last;
  r.bits_ok = r.words * 32 <= THREADS_MAX;             // one lane a bit slot in the ballot kernels
  // positions and counts are ints: N < 2^31 (so M is one too)
  r.ok = (long)Hs * Ws <= MASK_INT_LIMIT && (long)B * r.bpi * 256 <= THREADS_MAX;
  return r;
}

int mask_bits_launch(const RlePlan& r, const unsigned char* mask, unsigned int* bits, int Ws, hipStream_t stream) {
  hipLaunchKernelGGL(mask_bits_kernel, dim3(cdiv(r.words, 8)), dim3(256), 0, stream, mask, bits, Ws, (int)r.P, r.words);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

// zeroed counts, then count, scan, store
int rle_launch(const RlePlan& r, const unsigned int* bits, long long* stats, int* counts, int* s, int B, int Hs, int Ws, int cap,
               hipStream_t stream) {
  const hipError_t e = hipMemsetAsync(counts, 0, sizeof(int) * (size_t)B * cap, stream);
  if (e != hipSuccess) return (int)e;
  const dim3 grid((unsigned)(B * r.bpi));
  hipLaunchKernelGGL(rle_walk_kernel<false>, grid, dim3(256), 0, stream, bits, s + r.cnt, s + r.last, s + r.st, counts, Hs, Ws, (int)r.P,
                     (int)r.S, (int)r.bpi, cap);
  FS_LAUNCH_CHECK();
  hipLaunchKernelGGL(rle_scan_kernel, dim3((unsigned)B), dim3(256), 0, stream, s + r.cnt, s + r.last, s + r.st, stats, counts, Hs, Ws, (int)r.S,
                     cap);
  FS_LAUNCH_CHECK();
  hipLaunchKernelGGL(rle_walk_kernel<true>, grid, dim3(256), 0, stream, bits, s + r.cnt, s + r.last, s + r.st, counts, Hs, Ws, (int)r.P,
                     (int)r.S, (int)r.bpi, cap);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

extern "C" {

int fs_mask_bits(const unsigned char* mask, unsigned int* bits, int B, int Hs, int Ws, hipStream_t stream) {
  const RlePlan r = rle_plan(B, Hs, Ws);
  FS_REQUIRE(mask && bits && r.bits_ok);
  return mask_bits_launch(r, mask, bits, Ws, stream);
}

long fs_mask_rle_scratch_ints(int B, int Hs, int Ws) { return rle_plan(B, Hs, Ws).total; }
int fs_mask_rle(const unsigned int* bits, long long* stats, int* counts, int* scratch, int B, int Hs, int Ws, int cap, hipStream_t stream) {
  const RlePlan r = rle_plan(B, Hs, Ws);
  FS_REQUIRE(bits && stats && counts && scratch && r.ok && cap >= 1);
  return rle_launch(r, bits, stats, counts, scratch, B, Hs, Ws, cap, stream);
}

}  // extern "C"
