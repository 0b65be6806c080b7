// Morphology on bit words: erosion by a (2d+1)^2 square and the six pair counters of mask IoU / Boundary IoU (fs_mask_erode,
// fs_mask_pair_counts; no counterpart in the reference: UNPINNED, restated from the published definition of Boundary IoU, Cheng et al.,
// CVPR 2021).  All of it is integer work on bit words (mask_words.h: the layout).
//   E_d(m)[y,x] = 1 iff every pixel of the (2d+1) x (2d+1) square centred on (y,x) is set, pixels outside the image unset.
// The square is separable, and an AND over a run of L = 2d+1 positions is built by doubling: A_1 = m, A_2k[x] = A_k[x] & A_k[x+k]
// (the run x .. x+2k-1), and for the largest power of two k <= L, A_L[x] = A_k[x] & A_k[x+L-k]; the erosion is A_L[x-d].  Passes:
//   rows   a workgroup holds a few whole rows of words in LDS and doubles along the bit stream of each: word c of the next stage is
//          (32 bits of the stream from bit 32c) & (32 bits from bit 32c+k), a funnel shift over the word border; what lies left of
//          bit 0 or right of the last word reads as 0, and the input's bits at x >= Ws are cleared on load.  -> plane H in scratch
//   cols   a workgroup holds a tile of H -- Cw word columns, T output rows and d rows of halo above and below, rows outside the image 0
//          -- and doubles down the rows, whole words at a time.  -> out
//   count  (pair counts) popcounts of a&b, a, b and of the three bands m & ~E_d(m): shuffles in the wave, LDS across the waves, one
//          record of six ints a workgroup, then one workgroup per image adds its records in index order.  No atomics.
// With 2d+1 above a side the erosion is empty: out is cleared (the band is the mask) and neither pass runs.
#include "mask_words.h"

namespace {

constexpr int MORPH_THREADS = 256;
constexpr int MORPH_MAX_D = 2047;                      // 2d+1 rows of halo and one output row fit MORPH_LDS_WORDS at one word column
constexpr int MORPH_LDS_WORDS = 4096;                  // words a stage; two stages (ping and pong) are 32 KiB of static LDS
constexpr int MORPH_ROW_WORDS = 1024;                  // words a workgroup of the rows pass takes, where a row is shorter than that
constexpr int MORPH_COUNT_WORDS = 4096;                // words a workgroup of the count pass takes: 2^17 bits, a record fits an int
constexpr int MORPH_REC = 6;

struct MorphPlan {
  int P, R, tiles_r;                                   // rows pass: R rows a workgroup
  int Cw, T, tiles_y, tiles_c;                         // cols pass: Cw word columns by T output rows a workgroup
  int chunks;                                          // count pass: workgroups an image
  bool empty, ok;                                      // empty: 2d+1 > min(Hs, Ws)
  long words;                                          // Hs * P
};

MorphPlan morph_plan(int B, int Hs, int Ws, int d) {
  MorphPlan p = {};
  if (!(B > 0 && Hs > 0 && Ws > 0 && Hs <= MASK_MAX_SIDE && Ws <= MASK_MAX_SIDE && (long)Hs * Ws < MASK_INT_LIMIT && d >= 1 &&
        d <= MORPH_MAX_D))
    return p;
  p.P = mask_row_words(Ws);
  p.words = (long)Hs * p.P;
  p.empty = 2L * d + 1 > (Hs < Ws ? Hs : Ws);
  p.R = MORPH_ROW_WORDS / p.P > 0 ? MORPH_ROW_WORDS / p.P : 1;
  if (p.R > Hs) p.R = Hs;
  p.tiles_r = (Hs + p.R - 1) / p.R;
  // the widest tile of up to 32 word columns whose halo is at most half of its rows; one column where d is that large
  int Cw = 32;
  while (Cw > 1 && (Cw / 2 >= p.P || MORPH_LDS_WORDS / Cw < 4 * d + 2)) Cw >>= 1;
  p.Cw = Cw;
  p.T = MORPH_LDS_WORDS / Cw - 2 * d;                  // >= 2: d <= MORPH_MAX_D
  if (p.T > Hs) p.T = Hs;
  p.tiles_y = (Hs + p.T - 1) / p.T;
  p.tiles_c = (p.P + Cw - 1) / Cw;
  p.chunks = (int)((p.words + MORPH_COUNT_WORDS - 1) / MORPH_COUNT_WORDS);
  // every grid is images * tiles workgroups in x, for up to 2 B images
  const long most = (long)p.tiles_y * p.tiles_c > p.tiles_r ? (long)p.tiles_y * p.tiles_c : p.tiles_r;
  p.ok = 2L * B * (most > p.chunks ? most : p.chunks) < MASK_INT_LIMIT && 2L * B * p.words < (1L << 40);
  return p;
}

// image i of a launch over 2 B images: the first B are a's, the rest b's
__device__ __forceinline__ const unsigned int* morph_src(const unsigned int* a, const unsigned int* b, int B, int img, size_t words) {
  return img < B ? a + (size_t)img * words : b + (size_t)(img - B) * words;
}

// H[img] = the AND of each row's 2d+1 neighbours along x.  grid = images * tiles_r, R rows of P words a workgroup (R * P <= 4096)
__global__ __launch_bounds__(MORPH_THREADS) void morph_rows_kernel(const unsigned int* __restrict__ a, const unsigned int* __restrict__ b,
                                                                   unsigned int* __restrict__ H, int B, int Hs, int Ws, int P, int R,
                                                                   int tiles, int d) {
  __shared__ unsigned int stage[2][MORPH_LDS_WORDS];
  const int img = blockIdx.x / tiles, tile = blockIdx.x - img * tiles;
  const size_t words = (size_t)Hs * P;
  const unsigned int* src = morph_src(a, b, B, img, words);
  unsigned int* dst = H + (size_t)img * words;
  const int y0 = tile * R;
  const int n = min(R, Hs - y0) * P;
  const size_t base = (size_t)y0 * P;
  for (int i = threadIdx.x; i < n; i += MORPH_THREADS) stage[0][i] = src[base + i] & mask_tail(i % P, P, Ws);
  __syncthreads();
  const int L = 2 * d + 1;
  int cur = 0, k = 1;
  for (; 2 * k <= L; k *= 2, cur ^= 1) {
    for (int i = threadIdx.x; i < n; i += MORPH_THREADS) {
      const int r = i / P, c = i - r * P;
      const unsigned int* row = stage[cur] + r * P;
      stage[cur ^ 1][i] = row[c] & mask_window<false>(row, P, Ws, 32 * c + k);
    }
    __syncthreads();
  }
  for (int i = threadIdx.x; i < n; i += MORPH_THREADS) {
    const int r = i / P, c = i - r * P;
    const unsigned int* row = stage[cur] + r * P;
    dst[base + i] = mask_window<false>(row, P, Ws, 32 * c - d) & mask_window<false>(row, P, Ws, 32 * c - d + L - k);
  }
}

// out[img] = the AND of each column's 2d+1 neighbours along y.  grid = images * tiles_y * tiles_c; the tile is rows y0-d .. y0+T-1+d
// of Cw word columns, (T + 2d) * Cw <= 4096 words
__global__ __launch_bounds__(MORPH_THREADS) void morph_cols_kernel(const unsigned int* __restrict__ H, unsigned int* __restrict__ out, int Hs,
                                                                   int P, int Cw, int T, int tiles_y, int tiles_c, int d) {
  __shared__ unsigned int stage[2][MORPH_LDS_WORDS];
  const int per = tiles_y * tiles_c;
  const int img = blockIdx.x / per, t = blockIdx.x - img * per;
  const int ty = t / tiles_c, tc = t - ty * tiles_c;
  const size_t words = (size_t)Hs * P;
  const unsigned int* src = H + (size_t)img * words;
  unsigned int* dst = out + (size_t)img * words;
  const int y0 = ty * T, c0 = tc * Cw;
  const int rows_out = min(T, Hs - y0), rows_in = rows_out + 2 * d;
  const int n = rows_in * Cw;
  for (int i = threadIdx.x; i < n; i += MORPH_THREADS) {
    const int r = i / Cw, cc = i - r * Cw;
    const int y = y0 - d + r, c = c0 + cc;
    stage[0][i] = (y >= 0 && y < Hs && c < P) ? src[(size_t)y * P + c] : 0u;
  }
  __syncthreads();
  const int L = 2 * d + 1;
  int cur = 0, k = 1;
  for (; 2 * k <= L; k *= 2, cur ^= 1) {
    for (int i = threadIdx.x; i < n; i += MORPH_THREADS) {
      const int j = i + k * Cw;                        // the same column k rows below; past the tile it feeds no output
      stage[cur ^ 1][i] = j < n ? stage[cur][i] & stage[cur][j] : 0u;
    }
    __syncthreads();
  }
  const int m = rows_out * Cw;
  for (int i = threadIdx.x; i < m; i += MORPH_THREADS) {
    const int r = i / Cw, cc = i - r * Cw;
    const int c = c0 + cc;
    if (c < P) dst[(size_t)(y0 + r) * P + c] = stage[cur][i] & stage[cur][i + (L - k) * Cw];      // row r + L - 1 <= rows_in - 1
  }
}

__global__ __launch_bounds__(MORPH_THREADS) void morph_clear_kernel(unsigned int* __restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * MORPH_THREADS + threadIdx.x;
  if (i < n) out[i] = 0u;
}

// rec[img][chunk] = the six popcounts over this workgroup's words; E (2 B images: a's erosions, then b's) null = the empty erosion
__global__ __launch_bounds__(MORPH_THREADS) void morph_count_kernel(const unsigned int* __restrict__ a, const unsigned int* __restrict__ b,
                                                                    const unsigned int* __restrict__ E, int* __restrict__ rec, int B, int Hs,
                                                                    int Ws, int P, int chunks) {
  __shared__ int red[MORPH_THREADS / 64][MORPH_REC];
  const int img = blockIdx.x / chunks, chunk = blockIdx.x - img * chunks;
  const size_t words = (size_t)Hs * P;
  const unsigned int* pa = a + (size_t)img * words;
  const unsigned int* pb = b + (size_t)img * words;
  const unsigned int* ea = E ? E + (size_t)img * words : nullptr;
  const unsigned int* eb = E ? E + (size_t)(B + img) * words : nullptr;
  const size_t i0 = (size_t)chunk * MORPH_COUNT_WORDS;
  const int n = (int)(words - i0 < (size_t)MORPH_COUNT_WORDS ? words - i0 : (size_t)MORPH_COUNT_WORDS);
  int v[MORPH_REC] = {0, 0, 0, 0, 0, 0};
  for (int i = threadIdx.x; i < n; i += MORPH_THREADS) {
    const size_t at = i0 + i;
    const unsigned int tail = mask_tail((int)(at % P), P, Ws);
    const unsigned int wa = pa[at] & tail, wb = pb[at] & tail;
    const unsigned int ba = ea ? wa & ~ea[at] : wa, bb = eb ? wb & ~eb[at] : wb;
    v[0] += __popc(wa & wb), v[1] += __popc(wa), v[2] += __popc(wb);
    v[3] += __popc(ba & bb), v[4] += __popc(ba), v[5] += __popc(bb);
  }
#pragma unroll
  for (int q = 0; q < MORPH_REC; ++q) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[q] += __shfl_xor(v[q], o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int q = 0; q < MORPH_REC; ++q) red[threadIdx.x >> 6][q] = v[q];
  }
  __syncthreads();
  if (threadIdx.x < MORPH_REC) {
    int s = 0;
    for (int w = 0; w < MORPH_THREADS / 64; ++w) s += red[w][threadIdx.x];
    rec[((size_t)img * chunks + chunk) * MORPH_REC + threadIdx.x] = s;
  }
}

// pair[img][q] = the sum of the image's records in index order: one wave an image, lane l takes records l, l + 64, ...
__global__ __launch_bounds__(64) void morph_sum_kernel(const int* __restrict__ rec, long long* __restrict__ pair, int chunks) {
  const size_t img = blockIdx.x;
  const int* r = rec + img * (size_t)chunks * MORPH_REC;
#pragma unroll
  for (int q = 0; q < MORPH_REC; ++q) {
    long long s = 0;
    for (int i = threadIdx.x; i < chunks; i += 64) s += r[(size_t)i * MORPH_REC + q];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (threadIdx.x == 0) pair[img * MORPH_REC + q] = s;
  }
}

// the erosions of n images (a's B, then b's n - B where n = 2 B) into E, through the plane H; the caller has checked p
int morph_erode_launch(const MorphPlan& p, const unsigned int* a, const unsigned int* b, unsigned int* H, unsigned int* E, int B, int n, int Hs,
                       int Ws, int d, hipStream_t stream) {
  hipLaunchKernelGGL(morph_rows_kernel, dim3((unsigned)(n * p.tiles_r)), dim3(MORPH_THREADS), 0, stream, a, b, H, B, Hs, Ws, p.P, p.R,
                     p.tiles_r, d);
  FS_LAUNCH_CHECK();
  hipLaunchKernelGGL(morph_cols_kernel, dim3((unsigned)(n * p.tiles_y * p.tiles_c)), dim3(MORPH_THREADS), 0, stream, (const unsigned int*)H, E,
                     Hs, p.P, p.Cw, p.T, p.tiles_y, p.tiles_c, d);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

}  // namespace

extern "C" {

long fs_mask_erode_scratch_ints(int B, int Hs, int Ws, int d) {
  const MorphPlan p = morph_plan(B, Hs, Ws, d);
  return p.ok ? (long)B * p.words : 0;
}

int fs_mask_erode(const unsigned int* bits, unsigned int* out, int* scratch, int B, int Hs, int Ws, int d, hipStream_t stream) {
  const MorphPlan p = morph_plan(B, Hs, Ws, d);
  FS_REQUIRE(bits && out && scratch && out != bits && p.ok);
  if (p.empty) {
    const size_t n = (size_t)B * p.words;
    hipLaunchKernelGGL(morph_clear_kernel, dim3((unsigned)((n + MORPH_THREADS - 1) / MORPH_THREADS)), dim3(MORPH_THREADS), 0, stream, out, n);
    FS_LAUNCH_CHECK();
    return FS_OK;
  }
  return morph_erode_launch(p, bits, bits, reinterpret_cast<unsigned int*>(scratch), out, B, B, Hs, Ws, d, stream);
}

// scratch: H (2 B planes), E (2 B planes), the records
long fs_mask_pair_scratch_ints(int B, int Hs, int Ws, int d) {
  const MorphPlan p = morph_plan(B, Hs, Ws, d);
  return p.ok ? 4L * B * p.words + (long)B * p.chunks * MORPH_REC : 0;
}

int fs_mask_pair_counts(const unsigned int* a, const unsigned int* b, long long* pair, int* scratch, int B, int Hs, int Ws, int d,
                        hipStream_t stream) {
  const MorphPlan p = morph_plan(B, Hs, Ws, d);
  FS_REQUIRE(a && b && pair && scratch && p.ok);
  unsigned int* H = reinterpret_cast<unsigned int*>(scratch);
  unsigned int* E = H + 2 * (size_t)B * p.words;
  int* rec = scratch + 4 * (size_t)B * p.words;
  if (!p.empty) FS_TRY(morph_erode_launch(p, a, b, H, E, B, 2 * B, Hs, Ws, d, stream));
  hipLaunchKernelGGL(morph_count_kernel, dim3((unsigned)(B * p.chunks)), dim3(MORPH_THREADS), 0, stream, a, b,
                     p.empty ? (const unsigned int*)nullptr : (const unsigned int*)E, rec, B, Hs, Ws, p.P, p.chunks);
  FS_LAUNCH_CHECK();
  hipLaunchKernelGGL(morph_sum_kernel, dim3((unsigned)B), dim3(64), 0, stream, (const int*)rec, pair, p.chunks);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

}  // extern "C"
