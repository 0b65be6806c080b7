// Global motion compensation in front of the gaze gate: carry a viewer's record along a translating camera (no counterpart in the
// reference: UNPINNED, a definition of this library's).  All of it is integer work.  Passes:
//   profiles the hot pass, 12 bytes a pixel: the integral projections of a frame, prof (B, H + W) int32 = [prow (H) | pcol (W)] of the
//            luma code L = q_r + q_g + q_b.  Cut along the rows as the gate's tile pass is: a workgroup takes 64 rows of a 256-column
//            segment, a lane four pixels of a row by 16-byte loads; row sums meet by shuffles, column sums stay in the lanes and meet
//            through LDS; both are added into prof with integer atomics, contiguous words a wave (any order gives the same integers),
//            prof zeroed before.
//   estimate a workgroup per viewer, one axis after the other, both profiles of the axis in LDS: the cost of every shift, then one lane
//            takes the least by the order of the definition and applies the gain rule.
//   move     for the viewers whose shift is not (0, 0) only -- every workgroup reads shift[b] and leaves otherwise: the key frame and
//            the mask's bit words are written, moved, into second buffers (the bits by funnel shifts over the word borders) and copied
//            back; one lane a viewer moves the gazes and the totals and writes the motion row; fs_mask_rle's passes re-encode the moved
//            words (mask_words.h: the layout) into scratch rows that reach stats / counts for the moving viewers alone; the key
//            profiles are taken again.
//   commit   for the viewers whose record was made anew: the frame's profiles become the key's, the totals 0.
// The pixel code q is the gate's, one function (frame_view.h).  A frame comes as planar fp32, planar bytes (pixel value byte / 255, q the
// byte: its profiles are fs_key_profiles of it) or interleaved bytes read where they lie; the profile pass and the move pass, which fills
// the key's uncovered border with the frame's codes, are written once over the frame's reader (frame_view.h), a kernel a layout where
// the layouts' arguments differ.  Every other pass reads no frame.
#include "mask_words.h"
#include "frame_view.h"

namespace {

constexpr long MOTION_INT_LIMIT = 2147483647L;
constexpr long MOTION_WGS_MAX = 16777215L;             // workgroups of 256 threads: fewer than 2^32 work-items a launch
constexpr int MOTION_MAX_SIDE = 1 << 26;               // the gaze in 1/16 pixels stays below 2^30, as in the gate
constexpr int MOTION_THREADS = 256;
constexpr int MOTION_SEG = 256;                        // columns a workgroup of the profile pass covers
constexpr int MOTION_BAND = 64;                        // rows a workgroup of the profile pass covers
constexpr int MOTION_MAX_R = 255;
constexpr int MOTION_LDS_BYTES = 65536;                // the estimate: two profiles of an axis and the costs
constexpr int MOTION_ITER = 16;                        // elements a lane of the move and copy passes takes, 256 lanes apart

__device__ __forceinline__ bool motion_still(const long long* __restrict__ shift, size_t b) {
  return shift[4 * b] == 0 && shift[4 * b + 1] == 0;
}

// prof[b] <- 0 for every viewer (shift null) or for the moving ones
__global__ __launch_bounds__(MOTION_THREADS) void motion_zero_kernel(int* __restrict__ prof, const long long* __restrict__ shift, int n,
                                                                     unsigned int bpv) {
  const size_t b = blockIdx.x / bpv;
  if (shift != nullptr && motion_still(shift, b)) return;
  const unsigned int i = (blockIdx.x - (unsigned int)b * bpv) * MOTION_THREADS + threadIdx.x;
  if (i < (unsigned int)n) prof[b * n + i] = 0;
}

// prof[b] += the row and column sums of L over one band of one segment, the frame read through its reader.  VEC (the reader's quad): a
// wave takes every fourth row, a lane four pixels of it -- their luma codes from aligned loads.  Otherwise a lane takes one column of the
// band.
template <class F, bool VEC>
__device__ __forceinline__ void motion_profile(const F& f, int* __restrict__ prof, int H, int W, int nseg, int nband) {
  __shared__ int red[MOTION_THREADS / 64][MOTION_SEG];
  __shared__ int rsum[MOTION_THREADS / 64][MOTION_BAND];   // row sums meet here, so that one wave adds the band's rows as contiguous words
  const unsigned int blk = blockIdx.x;
  const int seg = (int)(blk % (unsigned)nseg);
  const int band = (int)((blk / (unsigned)nseg) % (unsigned)nband);
  const size_t b = blk / (unsigned)nseg / (unsigned)nband;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int y0 = band * MOTION_BAND, rows = min(MOTION_BAND, H - y0);
  int* prow = prof + b * ((size_t)H + W) + y0;
  int* pcol = prof + b * ((size_t)H + W) + H;
  if (VEC) {
    const int x = seg * MOTION_SEG + lane * 4;
    const auto base = f.px(b, y0, x);
    int acc[4] = {0, 0, 0, 0};
    for (int r = wave; r < rows; r += MOTION_THREADS / 64) {
      int l[4] = {0, 0, 0, 0};
      if (x < W) f.luma4(f.down(base, r), l);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] += l[j];
      const int rs = wave_sum_i(l[0] + l[1] + l[2] + l[3]);
      if (lane == 0) rsum[0][r] = rs;                   // a row is one wave's
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) red[wave][lane * 4 + j] = acc[j];
    __syncthreads();
    if ((int)threadIdx.x < rows) atomicAdd(prow + threadIdx.x, rsum[0][threadIdx.x]);
    const int xc = seg * MOTION_SEG + (int)threadIdx.x;
    if (xc < W) atomicAdd(pcol + xc, red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x]);
  } else {
    const int x = seg * MOTION_SEG + (int)threadIdx.x;
    const auto base = f.px(b, y0, x);
    int acc = 0;
    for (int r = 0; r < rows; ++r) {
      int l = 0;
      if (x < W) {
        const auto at = f.down(base, r);
        l = f.code(at, 0) + f.code(at, 1) + f.code(at, 2);
      }
      acc += l;
      const int rs = wave_sum_i(l);
      if (lane == 0) rsum[wave][r] = rs;
    }
    __syncthreads();
    if ((int)threadIdx.x < rows)
      atomicAdd(prow + threadIdx.x, rsum[0][threadIdx.x] + rsum[1][threadIdx.x] + rsum[2][threadIdx.x] + rsum[3][threadIdx.x]);
    if (x < W) atomicAdd(pcol + x, acc);
  }
}

// its kernels: each layout keeps the parameters of its entry point and builds its reader from them.  Only a planar frame can be a key,
// whose profiles are taken again after a move: shift null, every viewer; else the moving ones, and a still viewer's workgroups leave here.
template <typename T, bool VEC>
__global__ __launch_bounds__(MOTION_THREADS) void motion_profile_kernel(const T* __restrict__ src, const long long* __restrict__ shift,
                                                                        int* __restrict__ prof, int H, int W, int nseg, int nband) {
  if (shift != nullptr && motion_still(shift, blockIdx.x / (unsigned)nseg / (unsigned)nband)) return;
  motion_profile<PlanarFrame<T>, VEC>(PlanarFrame<T>(src, H, W), prof, H, W, nseg, nband);
}
template <int SX, bool VEC>
__global__ __launch_bounds__(MOTION_THREADS) void motion_profile_hwc_kernel(const unsigned char* __restrict__ src, long sb, long sy,
                                                                            int* __restrict__ prof, int H, int W, int nseg, int nband) {
  motion_profile<HwcFrame<SX>, VEC>(HwcFrame<SX>(src, sb, sy, SX), prof, H, W, nseg, nband);
}

template <bool VEC>
__global__ __launch_bounds__(MOTION_THREADS) void motion_profile_nv12_kernel(const unsigned char* __restrict__ yp, const unsigned char* __restrict__ uvp,
                                                                             long sb, long sy, long ub, long uy, Nv12Csc k, int* __restrict__ prof,
                                                                             int H, int W, int nseg, int nband) {
  motion_profile<Nv12Frame, VEC>(Nv12Frame(yp, uvp, sb, sy, ub, uy, k), prof, H, W, nseg, nband);
}

// One workgroup a viewer.  For each axis: P, K of length n in LDS; cost[j] for s = j - R = sum_{i=R}^{n-1-R} |P[i] - K[i - s]|, a wave
// a shift; lane 0 takes the least, ties to the smaller |s|, then to the negative s, and keeps it only if cost * 8 <= cost(0) * gain.
__global__ __launch_bounds__(MOTION_THREADS) void motion_estimate_kernel(const int* __restrict__ pnew, const int* __restrict__ pkey,
                                                                         const long long* __restrict__ gstate, long long* __restrict__ shift,
                                                                         int H, int W, int R, int gain) {
  extern __shared__ long long motion_lds[];
  const size_t b = blockIdx.x;
  long long* o = shift + b * 4;
  if (gstate[b * 6] == 0) {                            // no record: nothing to carry
    if (threadIdx.x < 4) o[threadIdx.x] = 0;
    return;
  }
  const int ns = 2 * R + 1;
  long long* cost = motion_lds;
  int* P = reinterpret_cast<int*>(motion_lds + ns);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long long best_sum = 0, zero_sum = 0;
  int d0 = 0, d1 = 0;
  for (int axis = 0; axis < 2; ++axis) {
    const int n = axis == 0 ? H : W;
    int* K = P + n;
    const size_t at = b * ((size_t)H + W) + (axis == 0 ? 0 : H);
    for (int i = threadIdx.x; i < n; i += MOTION_THREADS) {
      P[i] = pnew[at + i];
      K[i] = pkey[at + i];
    }
    __syncthreads();
    for (int j = wave; j < ns; j += MOTION_THREADS / 64) {
      const int s = j - R;
      long long c = 0;
      for (int i = R + lane; i <= n - 1 - R; i += 64) {
        const int v = P[i] - K[i - s];
        c += v < 0 ? -v : v;
      }
      c = wave_sum_ll(c);
      if (lane == 0) cost[j] = c;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int s_best = 0;
      long long c_best = cost[R];
      for (int a = 1; a <= R; ++a) {
        if (cost[R - a] < c_best) c_best = cost[R - a], s_best = -a;
        if (cost[R + a] < c_best) c_best = cost[R + a], s_best = a;
      }
      best_sum += c_best;
      zero_sum += cost[R];
      const int taken = (c_best * 8 <= cost[R] * gain) ? s_best : 0;
      if (axis == 0) d0 = taken;
      else d1 = taken;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    o[0] = d0;
    o[1] = d1;
    o[2] = best_sum;
    o[3] = zero_sum;
  }
}

// The workgroups of a viewer in the move and copy passes: nk over the key's bytes (V of them a lane, MOTION_ITER times), then nb over the
// bit words (one a lane).
// bits2[y,x] = bits[y-dy,x-dx] where that lies in the frame, else 0: word w of viewer b, by a funnel shift over the word border
__device__ __forceinline__ void motion_move_bits(const unsigned int* __restrict__ bits, unsigned int* __restrict__ bits2, size_t b, unsigned int w,
                                                 int dy, int dx, int H, int W, int P) {
  if (w >= (unsigned int)(H * P)) return;
  const int y = (int)(w / (unsigned)P), c = (int)(w - (unsigned)y * P);
  const int sy = y - dy;
  unsigned int out = 0;
  if (sy >= 0 && sy < H) out = mask_window<true>(bits + (b * H + sy) * P, P, W, 32 * c - dx) & mask_tail(c, P, W);
  bits2[b * H * P + w] = out;
}

// key2[c,y,x] = key[c,y-dy,x-dx] where that lies in the frame, else the code of the frame's (c,y,x), read through its reader; the bit
// words as above.
template <class F, int V>
__device__ __forceinline__ void motion_move(const F& f, const long long* __restrict__ shift, const unsigned char* __restrict__ key,
                                            unsigned char* __restrict__ key2, const unsigned int* __restrict__ bits,
                                            unsigned int* __restrict__ bits2, int H, int W, int P, unsigned int nk, unsigned int nb) {
  const size_t b = blockIdx.x / (nk + nb);
  const unsigned int r = blockIdx.x - (unsigned int)b * (nk + nb);
  const int dy = (int)shift[4 * b], dx = (int)shift[4 * b + 1];
  if (r < nk) {
    const size_t plane = (size_t)H * W, per = 3 * plane;
    const unsigned char* kb = key + b * per;
    unsigned char* ob = key2 + b * per;
    for (int it = 0; it < MOTION_ITER; ++it) {
      const size_t e = (((size_t)r * MOTION_ITER + it) * MOTION_THREADS + threadIdx.x) * V;
      if (e >= per) return;
      const int c = (int)(e / plane);
      const int rem = (int)(e - c * plane);
      const int y = rem / W, x = rem - y * W;
      const int sy = y - dy;
      const bool row_in = sy >= 0 && sy < H;
      const size_t srow = c * plane + (size_t)(row_in ? sy : 0) * W;
      unsigned int out = 0;
#pragma unroll
      for (int j = 0; j < V; ++j) {                    // V == 4: W % 4 == 0, the four pixels lie in one row
        const int sx = x + j - dx;
        const unsigned int k = (row_in && sx >= 0 && sx < W) ? (unsigned int)kb[srow + sx] : (unsigned int)f.code_of(b, e + j, c, y, x + j);
        out |= k << (8 * j);
      }
      if (V == 4) *reinterpret_cast<unsigned int*>(ob + e) = out;
      else ob[e] = (unsigned char)out;
    }
  } else {
    motion_move_bits(bits, bits2, b, (r - nk) * MOTION_THREADS + threadIdx.x, dy, dx, H, W, P);
  }
}

// its kernels: each layout keeps the parameters of its entry point and builds its reader from them; a still viewer's workgroups leave here
template <typename T, int V>
__global__ __launch_bounds__(MOTION_THREADS) void motion_move_kernel(const T* __restrict__ img, const long long* __restrict__ shift,
                                                                     const unsigned char* __restrict__ key, unsigned char* __restrict__ key2,
                                                                     const unsigned int* __restrict__ bits, unsigned int* __restrict__ bits2,
                                                                     int H, int W, int P, unsigned int nk, unsigned int nb) {
  if (motion_still(shift, blockIdx.x / (nk + nb))) return;
  motion_move<PlanarFrame<T>, V>(PlanarFrame<T>(img, H, W), shift, key, key2, bits, bits2, H, W, P, nk, nb);
}
template <int V>
__global__ __launch_bounds__(MOTION_THREADS) void motion_move_hwc_kernel(const unsigned char* __restrict__ img, long sb, long sy, int sx,
                                                                         const long long* __restrict__ shift, const unsigned char* __restrict__ key,
                                                                         unsigned char* __restrict__ key2, const unsigned int* __restrict__ bits,
                                                                         unsigned int* __restrict__ bits2, int H, int W, int P, unsigned int nk,
                                                                         unsigned int nb) {
  if (motion_still(shift, blockIdx.x / (nk + nb))) return;
  motion_move<HwcFrame<0>, V>(HwcFrame<0>(img, sb, sy, sx), shift, key, key2, bits, bits2, H, W, P, nk, nb);
}

template <int V>
__global__ __launch_bounds__(MOTION_THREADS) void motion_move_nv12_kernel(const unsigned char* __restrict__ yp, const unsigned char* __restrict__ uvp,
                                                                          long sb, long sy, long ub, long uy, Nv12Csc k,
                                                                          const long long* __restrict__ shift, const unsigned char* __restrict__ key,
                                                                          unsigned char* __restrict__ key2, const unsigned int* __restrict__ bits,
                                                                          unsigned int* __restrict__ bits2, int H, int W, int P, unsigned int nk,
                                                                          unsigned int nb) {
  if (motion_still(shift, blockIdx.x / (nk + nb))) return;
  motion_move<Nv12Frame, V>(Nv12Frame(yp, uvp, sb, sy, ub, uy, k), shift, key, key2, bits, bits2, H, W, P, nk, nb);
}

// key <- key2 and bits <- bits2 for the moving viewers; lane 0 of a viewer's first workgroup moves its gazes and totals and writes its
// motion row (every viewer).  gstate (B,6) as the gate's; mstate (B,4) = (dy_total, dx_total, moves, path); motion (B,6) = (dy, dx,
// cost_best, cost_zero, dy_total, dx_total).
template <int V>
__global__ __launch_bounds__(MOTION_THREADS) void motion_back_kernel(const long long* __restrict__ shift, const unsigned char* __restrict__ key2,
                                                                     unsigned char* __restrict__ key, const unsigned int* __restrict__ bits2,
                                                                     unsigned int* __restrict__ bits, long long* __restrict__ gstate,
                                                                     long long* __restrict__ mstate, long long* __restrict__ motion, int H, int W,
                                                                     int P, unsigned int nk, unsigned int nb) {
  const size_t b = blockIdx.x / (nk + nb);
  const unsigned int r = blockIdx.x - (unsigned int)b * (nk + nb);
  const long long dy = shift[4 * b], dx = shift[4 * b + 1];
  if (r == 0 && threadIdx.x == 0) {
    long long* g = gstate + b * 6;
    long long* m = mstate + b * 4;
    if (dy != 0 || dx != 0) {
      const long long top_y = ((long long)H - 1) * 16, top_x = ((long long)W - 1) * 16;
      g[1] = min(max(g[1] + 16 * dy, 0LL), top_y);
      g[2] = min(max(g[2] + 16 * dx, 0LL), top_x);
      g[3] = min(max(g[3] + 16 * dy, 0LL), top_y);
      g[4] = min(max(g[4] + 16 * dx, 0LL), top_x);
      m[0] += dy;
      m[1] += dx;
      m[2] += 1;
      m[3] += (dy < 0 ? -dy : dy) + (dx < 0 ? -dx : dx);
    }
    long long* o = motion + b * 6;
    o[0] = dy;
    o[1] = dx;
    o[2] = shift[4 * b + 2];
    o[3] = shift[4 * b + 3];
    o[4] = m[0];
    o[5] = m[1];
  }
  if (dy == 0 && dx == 0) return;
  if (r < nk) {
    const size_t per = (size_t)3 * H * W;
    for (int it = 0; it < MOTION_ITER; ++it) {
      const size_t e = (((size_t)r * MOTION_ITER + it) * MOTION_THREADS + threadIdx.x) * V;
      if (e >= per) return;
      if (V == 4) *reinterpret_cast<unsigned int*>(key + b * per + e) = *reinterpret_cast<const unsigned int*>(key2 + b * per + e);
      else key[b * per + e] = key2[b * per + e];
    }
  } else {
    const unsigned int w = (r - nk) * MOTION_THREADS + threadIdx.x;
    if (w >= (unsigned int)(H * P)) return;
    bits[b * H * P + w] = bits2[b * H * P + w];
  }
}

// for the moving viewers: the re-encoded rows reach the record (stats 12 words, counts cap words), and the key profiles are zeroed for
// the profile pass that follows
__global__ __launch_bounds__(MOTION_THREADS) void motion_finish_kernel(const long long* __restrict__ shift, const unsigned int* __restrict__ stats2,
                                                                       const unsigned int* __restrict__ counts2, unsigned int* __restrict__ stats,
                                                                       unsigned int* __restrict__ counts, int* __restrict__ prof_key, int cap, int n,
                                                                       unsigned int bpv) {
  const size_t b = blockIdx.x / bpv;
  if (motion_still(shift, b)) return;
  unsigned int w = (blockIdx.x - (unsigned int)b * bpv) * MOTION_THREADS + threadIdx.x;
  if (w < 12u) {
    stats[b * 12 + w] = stats2[b * 12 + w];
    return;
  }
  w -= 12u;
  if (w < (unsigned int)cap) {
    counts[b * cap + w] = counts2[b * cap + w];
    return;
  }
  w -= (unsigned int)cap;
  if (w < (unsigned int)n) prof_key[b * n + w] = 0;
}

// for the viewers of idx: prof_key <- prof, mstate <- 0
__global__ __launch_bounds__(MOTION_THREADS) void motion_commit_kernel(const int* __restrict__ idx, const int* __restrict__ prof,
                                                                       int* __restrict__ prof_key, long long* __restrict__ mstate, int B, int n,
                                                                       unsigned int bpv) {
  const unsigned int j = blockIdx.x / bpv;
  const int b = idx[j];
  if (b < 0 || b >= B) return;                         // an index outside the batch writes nothing
  const unsigned int i = (blockIdx.x - j * bpv) * MOTION_THREADS + threadIdx.x;
  if (i < (unsigned int)n) prof_key[(size_t)b * n + i] = prof[(size_t)b * n + i];
  if (i < 4u) mstate[(size_t)b * 4 + i] = 0;
}

bool motion_sizes_ok(int B, int H, int W) {
  return B > 0 && H > 0 && W > 0 && (long)H * W < MOTION_INT_LIMIT && 765L * (H > W ? H : W) < MOTION_INT_LIMIT + 1L;
}
bool motion_range_ok(int H, int W, int R) { return R >= 1 && R <= MOTION_MAX_R && 4L * R < (H < W ? H : W); }

// the profile pass's launch by the frame's layout; vec = four pixels a lane
template <typename T>
void motion_profile_launch(const PlanarFrame<T>& f, bool vec, dim3 grid, hipStream_t stream, const long long* shift, int* prof, int H, int W,
                           int nseg, int nband) {
  const dim3 block(MOTION_THREADS);
  if (vec) hipLaunchKernelGGL((motion_profile_kernel<T, true>), grid, block, 0, stream, f.p, shift, prof, H, W, nseg, nband);
  else hipLaunchKernelGGL((motion_profile_kernel<T, false>), grid, block, 0, stream, f.p, shift, prof, H, W, nseg, nband);
}
void motion_profile_launch(const HwcFrame<0>& f, bool vec, dim3 grid, hipStream_t stream, const long long*, int* prof, int H, int W, int nseg,
                           int nband) {
  const dim3 block(MOTION_THREADS);
  if (f.sx == 3 && vec) hipLaunchKernelGGL((motion_profile_hwc_kernel<3, true>), grid, block, 0, stream, f.p, f.sb, f.sy, prof, H, W, nseg, nband);
  else if (f.sx == 3) hipLaunchKernelGGL((motion_profile_hwc_kernel<3, false>), grid, block, 0, stream, f.p, f.sb, f.sy, prof, H, W, nseg, nband);
  else if (vec) hipLaunchKernelGGL((motion_profile_hwc_kernel<4, true>), grid, block, 0, stream, f.p, f.sb, f.sy, prof, H, W, nseg, nband);
  else hipLaunchKernelGGL((motion_profile_hwc_kernel<4, false>), grid, block, 0, stream, f.p, f.sb, f.sy, prof, H, W, nseg, nband);
}

void motion_profile_launch(const Nv12Frame& f, bool vec, dim3 grid, hipStream_t stream, const long long*, int* prof, int H, int W, int nseg,
                           int nband) {
  const dim3 block(MOTION_THREADS);
  if (vec) hipLaunchKernelGGL(motion_profile_nv12_kernel<true>, grid, block, 0, stream, f.yp, f.uvp, f.sb, f.sy, f.ub, f.uy, f.k, prof, H, W, nseg, nband);
  else hipLaunchKernelGGL(motion_profile_nv12_kernel<false>, grid, block, 0, stream, f.yp, f.uvp, f.sb, f.sy, f.ub, f.uy, f.k, prof, H, W, nseg, nband);
}

// fs_frame_profiles / fs_key_profiles / fs_frame_profiles_hwc / fs_frame_profiles_nv12: the checks, prof zeroed, the profile pass on every viewer
template <class F>
int motion_profiles(const F& f, int* prof, int B, int H, int W, hipStream_t stream) {
  FS_REQUIRE(f && prof && motion_sizes_ok(B, H, W) && f.ok(B, H, W));
  const int n = H + W;
  const int bpv = cdiv(n, MOTION_THREADS), nseg = cdiv(W, MOTION_SEG), nband = cdiv(H, MOTION_BAND);
  FS_REQUIRE((long)B * bpv <= MOTION_WGS_MAX && (long)B * nseg * nband <= MOTION_WGS_MAX);
  hipLaunchKernelGGL(motion_zero_kernel, dim3((unsigned)(B * bpv)), dim3(MOTION_THREADS), 0, stream, prof, (const long long*)nullptr, n,
                     (unsigned)bpv);
  FS_LAUNCH_CHECK();
  motion_profile_launch(f, f.quad(W), dim3((unsigned)(B * nseg * nband)), stream, nullptr, prof, H, W, nseg, nband);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

long motion_pad2(long v) { return (v + 1) & ~1L; }

// the move pass's launch by the frame's layout
template <int V, typename T>
void motion_move_launch(const PlanarFrame<T>& f, const long long* shift, const unsigned char* key, unsigned char* key2, const unsigned int* bits,
                        unsigned int* bits2, int H, int W, int P, long nk, long nb, dim3 grid, hipStream_t stream) {
  hipLaunchKernelGGL((motion_move_kernel<T, V>), grid, dim3(MOTION_THREADS), 0, stream, f.p, shift, key, key2, bits, bits2, H, W, P, (unsigned)nk,
                     (unsigned)nb);
}
template <int V>
void motion_move_launch(const HwcFrame<0>& f, const long long* shift, const unsigned char* key, unsigned char* key2, const unsigned int* bits,
                        unsigned int* bits2, int H, int W, int P, long nk, long nb, dim3 grid, hipStream_t stream) {
  hipLaunchKernelGGL(motion_move_hwc_kernel<V>, grid, dim3(MOTION_THREADS), 0, stream, f.p, f.sb, f.sy, f.sx, shift, key, key2, bits, bits2, H, W, P,
                     (unsigned)nk, (unsigned)nb);
}

template <int V>
void motion_move_launch(const Nv12Frame& f, const long long* shift, const unsigned char* key, unsigned char* key2, const unsigned int* bits,
                        unsigned int* bits2, int H, int W, int P, long nk, long nb, dim3 grid, hipStream_t stream) {
  hipLaunchKernelGGL(motion_move_nv12_kernel<V>, grid, dim3(MOTION_THREADS), 0, stream, f.yp, f.uvp, f.sb, f.sy, f.ub, f.uy, f.k, shift, key, key2, bits,
                     bits2, H, W, P, (unsigned)nk, (unsigned)nb);
}

// fs_state_shift / fs_state_shift_u8 / fs_state_shift_hwc / fs_state_shift_nv12: the checks and every pass, the move pass of the frame's layout
template <class F>
int motion_state_shift(const F& img, const long long* shift, unsigned char* key, unsigned char* key2, unsigned int* bits, unsigned int* bits2,
                       long long* gstate, long long* stats, int* counts, int* prof_key, long long* mstate, long long* motion, int* scratch, int B,
                       int H, int W, int cap, hipStream_t stream) {
  FS_REQUIRE(img && shift && key && key2 && bits && bits2 && gstate && stats && counts && prof_key && mstate && motion && scratch);
  FS_REQUIRE(motion_sizes_ok(B, H, W) && cap >= 1 && H <= MOTION_MAX_SIDE && W <= MOTION_MAX_SIDE && key != key2 && bits != bits2);
  const RlePlan rp = rle_plan(B, H, W);
  FS_REQUIRE(((uintptr_t)scratch & 7) == 0 && rp.total > 0 && img.ok(B, H, W));
  const int P = mask_row_words(W), n = H + W;
  const size_t per = (size_t)3 * H * W;
  const bool vec = W % 4 == 0 && ((uintptr_t)key & 3) == 0 && ((uintptr_t)key2 & 3) == 0;
  const long chunk = (long)MOTION_THREADS * MOTION_ITER * (vec ? 4 : 1);
  const long nk = (long)((per + chunk - 1) / chunk), nb = cdiv((long)H * P, MOTION_THREADS);
  const long bpv = cdiv(12L + cap + n, MOTION_THREADS);
  FS_REQUIRE((long)B * (nk + nb) <= MOTION_WGS_MAX && (long)B * bpv <= MOTION_WGS_MAX && 12L + cap + n < MOTION_INT_LIMIT);
  FS_REQUIRE((long)B * cdiv(n, MOTION_THREADS) <= MOTION_WGS_MAX && (long)B * cdiv(W, MOTION_SEG) * cdiv(H, MOTION_BAND) <= MOTION_WGS_MAX);
  long long* stats2 = reinterpret_cast<long long*>(scratch);
  int* counts2 = scratch + 12L * B;
  int* rle = counts2 + motion_pad2((long)B * cap);
  const dim3 grid((unsigned)(B * (nk + nb))), block(MOTION_THREADS);
  if (vec) {
    motion_move_launch<4>(img, shift, key, key2, bits, bits2, H, W, P, nk, nb, grid, stream);
    FS_LAUNCH_CHECK();
    hipLaunchKernelGGL(motion_back_kernel<4>, grid, block, 0, stream, shift, key2, key, bits2, bits, gstate, mstate, motion, H, W, P, (unsigned)nk,
                       (unsigned)nb);
  } else {
    motion_move_launch<1>(img, shift, key, key2, bits, bits2, H, W, P, nk, nb, grid, stream);
    FS_LAUNCH_CHECK();
    hipLaunchKernelGGL(motion_back_kernel<1>, grid, block, 0, stream, shift, key2, key, bits2, bits, gstate, mstate, motion, H, W, P, (unsigned)nk,
                       (unsigned)nb);
  }
  FS_LAUNCH_CHECK();
  FS_REQUIRE(rp.ok);
  FS_TRY(rle_launch(rp, bits, stats2, counts2, rle, B, H, W, cap, stream));
  hipLaunchKernelGGL(motion_finish_kernel, dim3((unsigned)(B * bpv)), block, 0, stream, shift, reinterpret_cast<const unsigned int*>(stats2),
                     reinterpret_cast<const unsigned int*>(counts2), reinterpret_cast<unsigned int*>(stats), reinterpret_cast<unsigned int*>(counts),
                     prof_key, cap, n, (unsigned)bpv);
  FS_LAUNCH_CHECK();
  const int nseg = cdiv(W, MOTION_SEG), nband = cdiv(H, MOTION_BAND);
  motion_profile_launch(PlanarFrame<unsigned char>(key, H, W), vec, dim3((unsigned)(B * nseg * nband)), stream, shift, prof_key, H, W, nseg, nband);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

}  // namespace

extern "C" {

int fs_frame_profiles(const float* img, int* prof, int B, int H, int W, hipStream_t stream) {
  return motion_profiles(PlanarFrame<float>(img, H, W), prof, B, H, W, stream);
}

int fs_key_profiles(const unsigned char* key, int* prof, int B, int H, int W, hipStream_t stream) {
  return motion_profiles(PlanarFrame<unsigned char>(key, H, W), prof, B, H, W, stream);
}

int fs_frame_profiles_hwc(const unsigned char* img, long sb, long sy, int sx, int* prof, int B, int H, int W, hipStream_t stream) {
  return motion_profiles(HwcFrame<0>(img, sb, sy, sx), prof, B, H, W, stream);
}

int fs_frame_profiles_nv12(const unsigned char* yp, const unsigned char* uvp, long sb, long sy, long ub, long uy, int yo, int yg, int rv, int gu,
                           int gv, int bu, int* prof, int B, int H, int W, hipStream_t stream) {
  return motion_profiles(Nv12Frame(yp, uvp, sb, sy, ub, uy, Nv12Csc{yo, yg, rv, gu, gv, bu}), prof, B, H, W, stream);
}

int fs_profile_shift(const int* prof, const int* prof_key, const long long* gstate, long long* shift, int B, int H, int W, int R, int gain,
                     hipStream_t stream) {
  FS_REQUIRE(prof && prof_key && gstate && shift && motion_sizes_ok(B, H, W) && B <= MOTION_WGS_MAX);
  FS_REQUIRE(motion_range_ok(H, W, R) && gain >= 0 && gain <= 8);
  const long lds = 8L * (2 * R + 1) + 8L * (H > W ? H : W);
  FS_REQUIRE(lds <= MOTION_LDS_BYTES);
  hipLaunchKernelGGL(motion_estimate_kernel, dim3((unsigned)B), dim3(MOTION_THREADS), (size_t)lds, stream, prof, prof_key, gstate, shift, H, W,
                     R, gain);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

long fs_state_shift_scratch_ints(int B, int H, int W, int cap) {
  if (!motion_sizes_ok(B, H, W) || cap < 1) return 0;
  return 12L * B + motion_pad2((long)B * cap) + rle_plan(B, H, W).total;
}

int fs_state_shift(const float* img, const long long* shift, unsigned char* key, unsigned char* key2, unsigned int* bits, unsigned int* bits2,
                   long long* gstate, long long* stats, int* counts, int* prof_key, long long* mstate, long long* motion, int* scratch, int B,
                   int H, int W, int cap, hipStream_t stream) {
  return motion_state_shift(PlanarFrame<float>(img, H, W), shift, key, key2, bits, bits2, gstate, stats, counts, prof_key, mstate, motion, scratch, B, H,
                            W, cap, stream);
}

int fs_state_shift_u8(const unsigned char* img, const long long* shift, unsigned char* key, unsigned char* key2, unsigned int* bits, unsigned int* bits2,
                      long long* gstate, long long* stats, int* counts, int* prof_key, long long* mstate, long long* motion, int* scratch, int B,
                      int H, int W, int cap, hipStream_t stream) {
  return motion_state_shift(PlanarFrame<unsigned char>(img, H, W), shift, key, key2, bits, bits2, gstate, stats, counts, prof_key, mstate, motion, scratch,
                            B, H, W, cap, stream);
}

int fs_state_shift_hwc(const unsigned char* img, long sb, long sy, int sx, const long long* shift, unsigned char* key, unsigned char* key2,
                       unsigned int* bits, unsigned int* bits2, long long* gstate, long long* stats, int* counts, int* prof_key, long long* mstate,
                       long long* motion, int* scratch, int B, int H, int W, int cap, hipStream_t stream) {
  return motion_state_shift(HwcFrame<0>(img, sb, sy, sx), shift, key, key2, bits, bits2, gstate, stats, counts, prof_key, mstate, motion, scratch, B, H,
                            W, cap, stream);
}

int fs_state_shift_nv12(const unsigned char* yp, const unsigned char* uvp, long sb, long sy, long ub, long uy, int yo, int yg, int rv, int gu, int gv,
                        int bu, const long long* shift, unsigned char* key, unsigned char* key2, unsigned int* bits, unsigned int* bits2,
                        long long* gstate, long long* stats, int* counts, int* prof_key, long long* mstate, long long* motion, int* scratch, int B,
                        int H, int W, int cap, hipStream_t stream) {
  return motion_state_shift(Nv12Frame(yp, uvp, sb, sy, ub, uy, Nv12Csc{yo, yg, rv, gu, gv, bu}), shift, key, key2, bits, bits2, gstate, stats, counts,
                            prof_key, mstate, motion, scratch, B, H, W, cap, stream);
}

int fs_motion_commit(const int* idx, int n, const int* prof, int* prof_key, long long* mstate, int B, int H, int W, hipStream_t stream) {
  FS_REQUIRE(prof && prof_key && mstate && motion_sizes_ok(B, H, W) && n >= 0 && n <= B && (n == 0 || idx != nullptr));
  if (n == 0) return FS_OK;
  const int len = H + W, bpv = cdiv(len, MOTION_THREADS);
  FS_REQUIRE((long)n * bpv <= MOTION_WGS_MAX);
  hipLaunchKernelGGL(motion_commit_kernel, dim3((unsigned)(n * bpv)), dim3(MOTION_THREADS), 0, stream, idx, prof, prof_key, mstate, B, len,
                     (unsigned)bpv);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

}  // extern "C"
