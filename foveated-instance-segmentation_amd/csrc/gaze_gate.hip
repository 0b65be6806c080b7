// The gaze gate: does the record a viewer already holds still answer "which instance is looked at" for a new frame and gaze?
// (no counterpart in the reference: UNPINNED, a definition of this library's).  All of it is integer work.  Passes:
//   tiles    the hot pass: the new frame against the 8-bit key frame the record was made from, one sum of absolute differences per
//            T x T tile.  15 bytes read per pixel, one int written per tile; every entry is one workgroup's and is stored plainly.
//   decide   a workgroup per viewer sums the tiles (changed tiles, changed tiles of the region of interest, total), one lane applies
//            the decision table.  Pure: it writes the gate record only.
//   commit   for the viewers that ran the network: the frame becomes the key frame, the gaze the key gaze, the new record's rows move to
//            the viewer's slots; every viewer's previous gaze and age advance.
// The pixel code q (frame_view.h) and the gaze in 1/16-pixel units (mask_words.h) are one function each, used by every pass that needs
// them: a frame against the key that commit made from it differs nowhere, NaN pixels included.
// A frame comes in four layouts -- planar fp32, planar bytes (pixel value byte / 255, whose code q is the byte; 6 bytes a pixel read
// instead of 15), interleaved bytes read where they lie, an NV12 surface read where it lies (4.5 bytes a pixel) -- and every pass that
// reads one is written once over the frame's reader (frame_view.h): the one-pixel tile pass for all four, the 16-pixel band for the three
// byte layouts (an interleaved frame's sixteen pixels are de-interleaved in registers, v_perm_b32, an NV12 frame's converted, so that
// v_sad_u8 meets matching bytes and the key stays planar).  The fp32 four-pixel band has a cut of its own.  Commit's frame pass is one
// template for the planar two, whose frames lie in the key's order, and a kernel each for the interleaved and the NV12 frame, which take
// pieces of rows through the reader.  A kernel a layout remains where the layouts' arguments differ; it builds its reader and calls the
// pass.  decide, and commit's state and row passes, read no frame.
#include "mask_words.h"
#include "frame_view.h"

namespace {

constexpr long GATE_INT_LIMIT = 2147483647L;           // pixel and tile indices are ints
constexpr long GATE_WGS_MAX = 16777215L;               // workgroups of 256 threads: fewer than 2^32 work-items a launch
constexpr int GATE_MAX_SIDE = 1 << 26;                 // decide / commit: the gaze in 1/16 pixels stays below 2^30, its squared distances below 2^62
constexpr int GATE_THREADS = 256;

__device__ __forceinline__ long long gate_d2(long long ay, long long ax, long long by, long long bx) {
  const long long dy = ay - by, dx = ax - bx;
  return dy * dy + dx * dx;
}

__device__ __forceinline__ int gate_absdiff(float v, unsigned int k) {
  const int d = pixel_q(v) - (int)k;
  return d < 0 ? -d : d;
}

constexpr int GATE_SEG = 256;                          // the four-pixel form: columns a workgroup covers, four a lane

// The four-pixel form (W % 4 == 0, img 16-byte and key 4-byte aligned): one workgroup per (viewer, tile row, 256-column segment).  A
// lane takes four pixels of a row -- a 16-byte load of img and a 4-byte load of key per channel -- so a wave reads 1 KB of one row at
// a time and the four waves take every fourth row of the band.  The T / 4 lanes of a tile are neighbours: their sums meet by
// shuffles, the four waves' through LDS, and one lane per tile stores the entry.
__global__ __launch_bounds__(GATE_THREADS) void gate_tiles_band_kernel(const float* __restrict__ img, const unsigned char* __restrict__ key,
                                                                       int* __restrict__ sad, int H, int W, int T, int th, int tw, int nseg) {
  __shared__ int red[GATE_THREADS / 64][GATE_SEG / 8];
  const unsigned int blk = blockIdx.x;
  const int seg = (int)(blk % (unsigned)nseg);
  const int ty = (int)((blk / (unsigned)nseg) % (unsigned)th);
  const size_t b = blk / (unsigned)nseg / (unsigned)th;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int y0 = ty * T, rows = min(T, H - y0);
  const int x = seg * GATE_SEG + lane * 4;
  const size_t plane = (size_t)H * W;
  int s = 0;
  if (x < W) {
    const size_t base = b * 3 * plane + (size_t)y0 * W + x;
#pragma unroll 2
    for (int r = wave; r < rows; r += GATE_THREADS / 64) {
      const size_t at = base + (size_t)r * W;
      f32x4 v[3];
      unsigned int k[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        v[c] = *reinterpret_cast<const f32x4*>(img + at + c * plane);
        k[c] = *reinterpret_cast<const unsigned int*>(key + at + c * plane);
      }
#pragma unroll
      for (int c = 0; c < 3; ++c)
        s += gate_absdiff(v[c].x, k[c] & 255u) + gate_absdiff(v[c].y, (k[c] >> 8) & 255u) + gate_absdiff(v[c].z, (k[c] >> 16) & 255u) +
             gate_absdiff(v[c].w, k[c] >> 24);
    }
  }
  const int lanes = T >> 2;                            // lanes a tile: 2, 4, 8 or 16
  for (int o = lanes >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((lane & (lanes - 1)) == 0) red[wave][lane / lanes] = s;
  __syncthreads();
  const int per_seg = GATE_SEG / T, tx = seg * per_seg + (int)threadIdx.x;
  if ((int)threadIdx.x < per_seg && tx < tw)
    sad[(b * th + ty) * tw + tx] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// The one-pixel form, for any layout, width and alignment: one workgroup per (viewer, tile row, tile column), a lane takes a pixel of the
// tile and reads its three channels through the frame's reader.
template <class F>
__device__ __forceinline__ void gate_tiles_px(const F& f, const unsigned char* __restrict__ key, int* __restrict__ sad, int H, int W, int T,
                                              int th, int tw) {
  __shared__ int red[GATE_THREADS / 64];
  const unsigned int blk = blockIdx.x;
  const int tx = (int)(blk % (unsigned)tw);
  const int ty = (int)((blk / (unsigned)tw) % (unsigned)th);
  const size_t b = blk / (unsigned)tw / (unsigned)th;
  const int y0 = ty * T, x0 = tx * T;
  const int rows = min(T, H - y0), cols = min(T, W - x0);
  const size_t plane = (size_t)H * W;
  const size_t base = b * 3 * plane + (size_t)y0 * W + x0;
  const auto fbase = f.px(b, y0, x0);
  int s = 0;
  const int per = rows * cols;
  for (int j = threadIdx.x; j < per; j += GATE_THREADS) {
    const int r = j / cols, x = j - r * cols;
    const size_t at = base + (size_t)r * W + x;
    const auto a = f.right(f.down(fbase, r), x);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int d = f.code(a, c) - (int)key[at + c * plane];
      s += d < 0 ? -d : d;
    }
  }
  s = wave_sum_i(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) sad[blk] = red[0] + red[1] + red[2] + red[3];
}

constexpr int GATE_SEG_U8 = 1024;                      // the byte form: the most columns a workgroup covers, sixteen a lane

// The 16-pixel form of the tile pass on a frame of bytes, planar or interleaved (the frame's vector form, key 16-byte aligned): the
// frame is bytes as the key is, the pixel code is the byte itself.  It keeps the band cut above: one workgroup per (viewer, tile row,
// segment), a lane takes sixteen pixels of a row -- the reader's sixteen bytes a channel in planar order and one 16-byte load of key per
// channel, four v_sad_u8 each, so that v_sad_u8 meets matching bytes -- and a lane's sixteen pixels are one tile's for T >= 16, two
// tiles' for T = 8 (s0 the first eight, s1 the last).  A row takes 1 << lg lanes, the least power of two that covers min(W, 1024)
// columns and is no less than a tile's lanes; the 64 >> lg rows of a wave are neighbours, the four waves take the row groups in turn.  A
// tile's lanes meet by shuffles inside a row, then across the rows of the wave, the waves through LDS.
template <class F>
__device__ __forceinline__ void gate_tiles_band(const F& f, const unsigned char* __restrict__ key, int* __restrict__ sad, int H, int W, int T,
                                                int th, int tw, int nseg, int lg) {
  __shared__ int red[GATE_THREADS / 64][GATE_SEG_U8 / 8];
  const unsigned int blk = blockIdx.x;
  const int seg = (int)(blk % (unsigned)nseg);
  const int ty = (int)((blk / (unsigned)nseg) % (unsigned)th);
  const size_t b = blk / (unsigned)nseg / (unsigned)th;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lpr = 1 << lg, sub = 64 >> lg;              // lanes a row, rows a wave
  const int cl = lane & (lpr - 1), rs = lane >> lg;
  const int y0 = ty * T, rows = min(T, H - y0);
  const int x = (seg << (lg + 4)) + cl * 16;
  const size_t plane = (size_t)H * W;
  unsigned int s0 = 0, s1 = 0;
  if (x < W) {
    const size_t base = b * 3 * plane + (size_t)y0 * W + x;
    const auto fbase = f.px(b, y0, x);
#pragma unroll 2
    for (int r = wave * sub + rs; r < rows; r += (GATE_THREADS / 64) * sub) {
      const size_t at = base + (size_t)r * W;
      u32x4 v[3], k[3];
      f.load16(f.down(fbase, r), v);
#pragma unroll
      for (int c = 0; c < 3; ++c) k[c] = *reinterpret_cast<const u32x4*>(key + at + c * plane);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        s0 = __builtin_amdgcn_sad_u8(v[c].x, k[c].x, s0);
        s0 = __builtin_amdgcn_sad_u8(v[c].y, k[c].y, s0);
        s1 = __builtin_amdgcn_sad_u8(v[c].z, k[c].z, s1);
        s1 = __builtin_amdgcn_sad_u8(v[c].w, k[c].w, s1);
      }
    }
  }
  int a0 = (int)s0, a1 = (int)s1;
  if (T >= 16) {
    a0 += a1;
    for (int o = (T >> 4) >> 1; o > 0; o >>= 1) a0 += __shfl_xor(a0, o, 64);      // the T / 16 lanes of a tile
  }
  for (int o = lpr; o < 64; o <<= 1) {                  // the rows of the wave
    a0 += __shfl_xor(a0, o, 64);
    a1 += __shfl_xor(a1, o, 64);
  }
  if (rs == 0) {
    if (T == 8) {
      red[wave][2 * cl] = a0;
      red[wave][2 * cl + 1] = a1;
    } else if ((cl & ((T >> 4) - 1)) == 0) {
      red[wave][cl / (T >> 4)] = a0;
    }
  }
  __syncthreads();
  const int per_seg = (lpr * 16) / T;                   // at most 128 entries a segment, one a lane
  const int tx = seg * per_seg + (int)threadIdx.x;
  if ((int)threadIdx.x < per_seg && tx < tw)
    sad[(b * th + ty) * tw + tx] = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
}

// The kernels of the two forms: each layout keeps the parameters of its entry point, raw pointers and scalars, and builds its reader from
// them (profiles/r33/README.md: a reader passed by value changes the device code).
__global__ __launch_bounds__(GATE_THREADS) void gate_tiles_kernel(const float* __restrict__ img, const unsigned char* __restrict__ key,
                                                                  int* __restrict__ sad, int H, int W, int T, int th, int tw) {
  gate_tiles_px(PlanarFrame<float>(img, H, W), key, sad, H, W, T, th, tw);
}
__global__ __launch_bounds__(GATE_THREADS) void gate_tiles_u8_kernel(const unsigned char* __restrict__ img, const unsigned char* __restrict__ key,
                                                                     int* __restrict__ sad, int H, int W, int T, int th, int tw) {
  gate_tiles_px(PlanarFrame<unsigned char>(img, H, W), key, sad, H, W, T, th, tw);
}
__global__ __launch_bounds__(GATE_THREADS) void gate_tiles_hwc_kernel(const unsigned char* __restrict__ img, long sb, long sy, int sx,
                                                                      const unsigned char* __restrict__ key, int* __restrict__ sad, int H, int W,
                                                                      int T, int th, int tw) {
  gate_tiles_px(HwcFrame<0>(img, sb, sy, sx), key, sad, H, W, T, th, tw);
}
__global__ __launch_bounds__(GATE_THREADS) void gate_tiles_u8_band_kernel(const unsigned char* __restrict__ img,
                                                                          const unsigned char* __restrict__ key, int* __restrict__ sad, int H,
                                                                          int W, int T, int th, int tw, int nseg, int lg) {
  gate_tiles_band(PlanarFrame<unsigned char>(img, H, W), key, sad, H, W, T, th, tw, nseg, lg);
}
template <int SX>
__global__ __launch_bounds__(GATE_THREADS) void gate_tiles_hwc_band_kernel(const unsigned char* __restrict__ img, long sb, long sy,
                                                                           const unsigned char* __restrict__ key, int* __restrict__ sad, int H,
                                                                           int W, int T, int th, int tw, int nseg, int lg) {
  gate_tiles_band(HwcFrame<SX>(img, sb, sy, SX), key, sad, H, W, T, th, tw, nseg, lg);
}

__global__ __launch_bounds__(GATE_THREADS) void gate_tiles_nv12_kernel(const unsigned char* __restrict__ yp, const unsigned char* __restrict__ uvp,
                                                                       long sb, long sy, long ub, long uy, Nv12Csc k,
                                                                       const unsigned char* __restrict__ key, int* __restrict__ sad, int H, int W,
                                                                       int T, int th, int tw) {
  gate_tiles_px(Nv12Frame(yp, uvp, sb, sy, ub, uy, k), key, sad, H, W, T, th, tw);
}
// a lane's sixteen converted pixels, four dwords a channel, meet the key's 16-byte loads as the byte frames' do
__global__ __launch_bounds__(GATE_THREADS) void gate_tiles_nv12_band_kernel(const unsigned char* __restrict__ yp, const unsigned char* __restrict__ uvp,
                                                                            long sb, long sy, long ub, long uy, Nv12Csc k,
                                                                            const unsigned char* __restrict__ key, int* __restrict__ sad, int H,
                                                                            int W, int T, int th, int tw, int nseg, int lg) {
  gate_tiles_band(Nv12Frame(yp, uvp, sb, sy, ub, uy, k), key, sad, H, W, T, th, tw, nseg, lg);
}

struct GateRule {
  int H, W, T, th, tw, P;
  int level, scene_tiles, roi_tiles, margin, max_age, inside_on;
  long long saccade2, fixation2;
};

// gstate (B,6) = (valid, gy_key, gx_key, gy_prev, gx_prev, age); stats (B,6) = fs_mask_rle's (area, x0, y0, bw, bh, n_runs);
// gate (B,8) = (code, n_changed, n_roi_changed, sad_total, d2_key, d2_prev, inside_bit, age + 1)
__global__ __launch_bounds__(GATE_THREADS) void gate_decide_kernel(const int* __restrict__ sad, const long long* __restrict__ gstate,
                                                                   const float* __restrict__ focus, const long long* __restrict__ stats,
                                                                   const unsigned int* __restrict__ bits, const int* __restrict__ force,
                                                                   long long* __restrict__ gate, GateRule p) {
  __shared__ int red_c[GATE_THREADS / 64], red_r[GATE_THREADS / 64];
  __shared__ long long red_t[GATE_THREADS / 64];
  const size_t b = blockIdx.x;
  const long long gy = mask_gaze16(focus[2 * b], p.H), gx = mask_gaze16(focus[2 * b + 1], p.W);
  const int py = mask_gaze_px(gy), px = mask_gaze_px(gx);
  const int gty = py / p.T, gtx = px / p.T;
  // the record's box grown by the margin and clipped, as a range of tiles; empty for an empty mask
  const long long* st = stats + b * 6;
  int tx0 = 1, tx1 = 0, ty0 = 1, ty1 = 0;
  if (st[0] != 0) {
    const long long bx0 = max(st[1] - p.margin, 0LL), bx1 = min(st[1] + st[3] + p.margin, (long long)p.W);
    const long long by0 = max(st[2] - p.margin, 0LL), by1 = min(st[2] + st[4] + p.margin, (long long)p.H);
    if (bx0 < bx1 && by0 < by1) {
      tx0 = (int)(bx0 / p.T), tx1 = (int)((bx1 - 1) / p.T);
      ty0 = (int)(by0 / p.T), ty1 = (int)((by1 - 1) / p.T);
    }
  }
  const int tiles = p.th * p.tw;
  const int* sb = sad + b * tiles;
  int nc = 0, nr = 0;
  long long tot = 0;
  for (int i = threadIdx.x; i < tiles; i += GATE_THREADS) {
    const int ty = i / p.tw, tx = i - ty * p.tw;
    const int n_el = 3 * min(p.T, p.H - ty * p.T) * min(p.T, p.W - tx * p.T);
    const int s = sb[i];
    const bool changed = s > p.level * n_el;
    const bool roi = (tx >= tx0 && tx <= tx1 && ty >= ty0 && ty <= ty1) || (tx == gtx && ty == gty);
    nc += changed ? 1 : 0;
    nr += (changed && roi) ? 1 : 0;
    tot += s;
  }
  nc = wave_sum_i(nc);
  nr = wave_sum_i(nr);
  tot = wave_sum_ll(tot);
  if ((threadIdx.x & 63) == 0) {
    red_c[threadIdx.x >> 6] = nc;
    red_r[threadIdx.x >> 6] = nr;
    red_t[threadIdx.x >> 6] = tot;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  nc = red_c[0] + red_c[1] + red_c[2] + red_c[3];
  nr = red_r[0] + red_r[1] + red_r[2] + red_r[3];
  tot = red_t[0] + red_t[1] + red_t[2] + red_t[3];
  const long long* g = gstate + b * 6;
  const long long valid = g[0], age1 = g[5] + 1;
  const long long d2_key = gate_d2(gy, gx, g[1], g[2]), d2_prev = gate_d2(gy, gx, g[3], g[4]);
  const int inside = (int)mask_bit(bits[(b * p.H + py) * p.P + (px >> 5)], px);
  int code = 0;
  if (force != nullptr && force[b] != 0) code = 7;
  else if (valid == 0) code = 1;
  else if (d2_prev > p.saccade2) code = 2;
  else if (nc > p.scene_tiles) code = 3;
  else if (nr > p.roi_tiles) code = 4;
  else if (!(p.inside_on != 0 && inside != 0) && d2_key > p.fixation2) code = 5;
  else if (p.max_age > 0 && age1 > p.max_age) code = 6;
  long long* o = gate + b * 8;
  o[0] = code;
  o[1] = nc;
  o[2] = nr;
  o[3] = tot;
  o[4] = d2_key;
  o[5] = d2_prev;
  o[6] = inside;
  o[7] = age1;
}

// is viewer b among idx[0 .. n), ascending?
__device__ __forceinline__ bool gate_ran(const int* __restrict__ idx, int n, int b) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (idx[mid] < b) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && idx[lo] == b;
}

// one lane per viewer: g_prev <- g for all; a viewer that ran gets g_key <- g, age <- 0, valid <- 1, any other age <- age + 1
__global__ void gate_commit_state_kernel(const int* __restrict__ idx, int n, long long* __restrict__ gstate, const float* __restrict__ focus,
                                         int B, int H, int W) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const long long gy = mask_gaze16(focus[2 * (size_t)b], H), gx = mask_gaze16(focus[2 * (size_t)b + 1], W);
  long long* g = gstate + (size_t)b * 6;
  if (n > 0 && gate_ran(idx, n, b)) {
    g[0] = 1;
    g[1] = gy;
    g[2] = gx;
    g[5] = 0;
  } else {
    g[5] = g[5] + 1;
  }
  g[3] = gy;
  g[4] = gx;
}

// key[idx[j]] <- the codes of img[idx[j]], a planar frame: it lies in the key's order, so a viewer is one run of per = 3 * H * W elements
// and bpi workgroups take it.  VEC (the reader's wide_commit, key aligned to the store): a lane takes four floats and stores their codes
// in 4 bytes, or copies sixteen bytes, whose codes they are; one element a lane otherwise.
template <typename T, bool VEC>
__global__ __launch_bounds__(GATE_THREADS) void gate_commit_frame_kernel(const T* __restrict__ img, const int* __restrict__ idx,
                                                                         unsigned char* __restrict__ key, int B, size_t per, unsigned int bpi) {
  const unsigned int j = blockIdx.x / bpi;
  const int b = idx[j];
  if (b < 0 || b >= B) return;                         // an index outside the batch writes nothing
  const size_t e = ((size_t)(blockIdx.x - j * bpi) * GATE_THREADS + threadIdx.x) * (VEC ? PlanarFrame<T>::lane : 1);
  if (e >= per) return;
  const size_t at = (size_t)b * per + e;
  if (!VEC) {
    key[at] = (unsigned char)pixel_q(img[at]);
  } else if (sizeof(T) == 4) {
    int q[4] = {0, 0, 0, 0};
    code4(img + at, q);
    *reinterpret_cast<unsigned int*>(key + at) = (unsigned int)q[0] | ((unsigned int)q[1] << 8) | ((unsigned int)q[2] << 16) | ((unsigned int)q[3] << 24);
  } else {
    *reinterpret_cast<u32x4*>(key + at) = *reinterpret_cast<const u32x4*>(img + at);
  }
}

// key[idx[j]] <- the de-interleaved frame of viewer idx[j] (fs_gate_commit_hwc); the key stays planar.  SX > 0, the vector form (the tile
// pass's conditions): a lane takes sixteen pixels of a row, splits them as the tile pass does and stores sixteen bytes a channel; per =
// H * W / 16 such pieces a viewer.  SX = 0, the one-byte form: per = 3 * H * W bytes a viewer, a lane one of them.
template <int SX>
__global__ __launch_bounds__(GATE_THREADS) void gate_commit_frame_hwc_kernel(const unsigned char* __restrict__ img, long sb, long sy, int sx,
                                                                             const int* __restrict__ idx, unsigned char* __restrict__ key, int B,
                                                                             int H, int W, size_t per, unsigned int bpi) {
  const unsigned int j = blockIdx.x / bpi;
  const int b = idx[j];
  if (b < 0 || b >= B) return;                         // an index outside the batch writes nothing
  const size_t e = (size_t)(blockIdx.x - j * bpi) * GATE_THREADS + threadIdx.x;
  if (e >= per) return;
  const HwcFrame<SX> f(img, sb, sy, sx);
  const size_t plane = (size_t)H * W;
  if (SX > 0) {
    const int w16 = W >> 4;
    const int y = (int)(e / (unsigned)w16), x = (int)(e - (size_t)y * w16) * 16;
    u32x4 v[3];
    f.load16(f.px(b, y, x), v);
#pragma unroll
    for (int c = 0; c < 3; ++c) *reinterpret_cast<u32x4*>(key + ((size_t)b * 3 + c) * plane + (size_t)y * W + x) = v[c];
  } else {
    const int c = (int)(e / plane);
    const size_t rem = e - c * plane;
    const int y = (int)(rem / (unsigned)W), x = (int)(rem - (size_t)y * W);
    key[(size_t)b * 3 * plane + e] = (unsigned char)f.code(f.px(b, y, x), c);
  }
}

// key[idx[j]] <- the converted frame of viewer idx[j] (fs_gate_commit_nv12); the key stays planar RGB bytes.  VEC, the vector form (the
// tile pass's conditions): a lane takes sixteen pixels of a row and stores sixteen bytes a channel; per = H * W / 16 such pieces a viewer.
// Otherwise per = 3 * H * W bytes a viewer, a lane one of them.
template <bool VEC>
__global__ __launch_bounds__(GATE_THREADS) void gate_commit_frame_nv12_kernel(const unsigned char* __restrict__ yp, const unsigned char* __restrict__ uvp,
                                                                              long sb, long sy, long ub, long uy, Nv12Csc k,
                                                                              const int* __restrict__ idx, unsigned char* __restrict__ key, int B,
                                                                              int H, int W, size_t per, unsigned int bpi) {
  const unsigned int j = blockIdx.x / bpi;
  const int b = idx[j];
  if (b < 0 || b >= B) return;                         // an index outside the batch writes nothing
  const size_t e = (size_t)(blockIdx.x - j * bpi) * GATE_THREADS + threadIdx.x;
  if (e >= per) return;
  const Nv12Frame f(yp, uvp, sb, sy, ub, uy, k);
  const size_t plane = (size_t)H * W;
  if (VEC) {
    const int w16 = W >> 4;
    const int y = (int)(e / (unsigned)w16), x = (int)(e - (size_t)y * w16) * 16;
    u32x4 v[3];
    f.load16(f.px(b, y, x), v);
#pragma unroll
    for (int c = 0; c < 3; ++c) *reinterpret_cast<u32x4*>(key + ((size_t)b * 3 + c) * plane + (size_t)y * W + x) = v[c];
  } else {
    const int c = (int)(e / plane);
    const size_t rem = e - c * plane;
    const int y = (int)(rem / (unsigned)W), x = (int)(rem - (size_t)y * W);
    key[(size_t)b * 3 * plane + e] = (unsigned char)f.code(f.px(b, y, x), c);
  }
}

// The record tensors as rows of 32-bit words (an int64 is two): cat 2, stats 12, counts cap, bits H * P, conf 3.  src == dst (or a
// null pair, conf) is a part of no words.
struct GateRows {
  const unsigned int* src[5];
  unsigned int* dst[5];
  unsigned int words[5];
  unsigned int total;
};

// row j of every part -> row idx[j]; bpr workgroups a row
__global__ __launch_bounds__(GATE_THREADS) void gate_commit_rows_kernel(const int* __restrict__ idx, int B, GateRows r, unsigned int bpr) {
  const unsigned int j = blockIdx.x / bpr;
  const int b = idx[j];
  if (b < 0 || b >= B) return;
  unsigned int w = (blockIdx.x - j * bpr) * GATE_THREADS + threadIdx.x;
  if (w >= r.total) return;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    if (w < r.words[k]) {
      r.dst[k][(size_t)b * r.words[k] + w] = r.src[k][(size_t)j * r.words[k] + w];
      return;
    }
    w -= r.words[k];
  }
}

bool gate_tile_ok(int T) { return T == 8 || T == 16 || T == 32 || T == 64; }
// a frame's vector form also asks the key to be aligned to what a lane takes of it: 4 bytes beside four floats, 16 beside sixteen bytes
template <class F>
bool gate_key_ok(const unsigned char* key) { return ((uintptr_t)key & (F::lane == 4 ? 3 : 15)) == 0; }

// the tile pass's launch on a frame of bytes, by its layout; band = the 16-pixel form
void gate_tiles_launch(const PlanarFrame<unsigned char>& f, bool band, dim3 grid, hipStream_t stream, const unsigned char* key, int* sad, int H, int W,
                       int T, int th, int tw, int nseg, int lg) {
  if (band) hipLaunchKernelGGL(gate_tiles_u8_band_kernel, grid, dim3(GATE_THREADS), 0, stream, f.p, key, sad, H, W, T, th, tw, nseg, lg);
  else hipLaunchKernelGGL(gate_tiles_u8_kernel, grid, dim3(GATE_THREADS), 0, stream, f.p, key, sad, H, W, T, th, tw);
}
void gate_tiles_launch(const HwcFrame<0>& f, bool band, dim3 grid, hipStream_t stream, const unsigned char* key, int* sad, int H, int W, int T, int th,
                       int tw, int nseg, int lg) {
  const dim3 block(GATE_THREADS);
  if (band && f.sx == 3) hipLaunchKernelGGL(gate_tiles_hwc_band_kernel<3>, grid, block, 0, stream, f.p, f.sb, f.sy, key, sad, H, W, T, th, tw, nseg, lg);
  else if (band) hipLaunchKernelGGL(gate_tiles_hwc_band_kernel<4>, grid, block, 0, stream, f.p, f.sb, f.sy, key, sad, H, W, T, th, tw, nseg, lg);
  else hipLaunchKernelGGL(gate_tiles_hwc_kernel, grid, block, 0, stream, f.p, f.sb, f.sy, f.sx, key, sad, H, W, T, th, tw);
}

void gate_tiles_launch(const Nv12Frame& f, bool band, dim3 grid, hipStream_t stream, const unsigned char* key, int* sad, int H, int W, int T, int th,
                       int tw, int nseg, int lg) {
  const dim3 block(GATE_THREADS);
  if (band)
    hipLaunchKernelGGL(gate_tiles_nv12_band_kernel, grid, block, 0, stream, f.yp, f.uvp, f.sb, f.sy, f.ub, f.uy, f.k, key, sad, H, W, T, th, tw, nseg, lg);
  else hipLaunchKernelGGL(gate_tiles_nv12_kernel, grid, block, 0, stream, f.yp, f.uvp, f.sb, f.sy, f.ub, f.uy, f.k, key, sad, H, W, T, th, tw);
}

// fs_gate_tiles_u8 / fs_gate_tiles_hwc / fs_gate_tiles_nv12: the checks, and the lanes a row and the segments of the 16-pixel form, chosen here alone
template <class F>
int gate_tiles_bytes(const F& f, const unsigned char* key, int* sad, int B, int H, int W, int T, hipStream_t stream) {
  FS_REQUIRE(f && key && sad && B > 0 && H > 0 && W > 0 && gate_tile_ok(T) && (long)H * W < GATE_INT_LIMIT && f.ok(B, H, W));
  const int th = cdiv(H, T), tw = cdiv(W, T);
  FS_REQUIRE((long)B * th * tw <= GATE_WGS_MAX);
  const bool band = f.wide(W) && gate_key_ok<F>(key);
  int lg = 0;                                           // lanes a row: covers min(W, 1024) columns, and a tile's T / 16 lanes
  while (lg < 6 && (16 << lg) < W) ++lg;
  while ((16 << lg) < T) ++lg;
  const int nseg = cdiv(W, 16 << lg);
  gate_tiles_launch(f, band, dim3((unsigned)((long)B * th * (band ? nseg : tw))), stream, key, sad, H, W, T, th, tw, nseg, lg);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

// the frame pass of commit by the frame's layout: a planar viewer is a run of per elements, an interleaved one H * W / 16 pieces (the
// vector form) or per bytes
template <typename T>
void gate_commit_frame(const PlanarFrame<T>& f, const int* idx, unsigned char* key, int B, int, int, size_t per, bool vec, long wgs, long bpi,
                       hipStream_t stream) {
  const dim3 grid((unsigned)wgs), block(GATE_THREADS);
  if (vec) hipLaunchKernelGGL((gate_commit_frame_kernel<T, true>), grid, block, 0, stream, f.p, idx, key, B, per, (unsigned)bpi);
  else hipLaunchKernelGGL((gate_commit_frame_kernel<T, false>), grid, block, 0, stream, f.p, idx, key, B, per, (unsigned)bpi);
}
void gate_commit_frame(const HwcFrame<0>& f, const int* idx, unsigned char* key, int B, int H, int W, size_t per, bool vec, long wgs, long bpi,
                       hipStream_t stream) {
  const dim3 grid((unsigned)wgs), block(GATE_THREADS);
  const size_t units = vec ? per / 48 : per;
  if (vec && f.sx == 3)
    hipLaunchKernelGGL(gate_commit_frame_hwc_kernel<3>, grid, block, 0, stream, f.p, f.sb, f.sy, f.sx, idx, key, B, H, W, units, (unsigned)bpi);
  else if (vec)
    hipLaunchKernelGGL(gate_commit_frame_hwc_kernel<4>, grid, block, 0, stream, f.p, f.sb, f.sy, f.sx, idx, key, B, H, W, units, (unsigned)bpi);
  else
    hipLaunchKernelGGL(gate_commit_frame_hwc_kernel<0>, grid, block, 0, stream, f.p, f.sb, f.sy, f.sx, idx, key, B, H, W, units, (unsigned)bpi);
}

void gate_commit_frame(const Nv12Frame& f, const int* idx, unsigned char* key, int B, int H, int W, size_t per, bool vec, long wgs, long bpi,
                       hipStream_t stream) {
  const dim3 grid((unsigned)wgs), block(GATE_THREADS);
  if (vec)
    hipLaunchKernelGGL(gate_commit_frame_nv12_kernel<true>, grid, block, 0, stream, f.yp, f.uvp, f.sb, f.sy, f.ub, f.uy, f.k, idx, key, B, H, W, per / 48,
                       (unsigned)bpi);
  else
    hipLaunchKernelGGL(gate_commit_frame_nv12_kernel<false>, grid, block, 0, stream, f.yp, f.uvp, f.sb, f.sy, f.ub, f.uy, f.k, idx, key, B, H, W, per,
                       (unsigned)bpi);
}

// fs_gate_commit / fs_gate_commit_u8 / fs_gate_commit_hwc / fs_gate_commit_nv12: the checks, the state pass, the frame pass of the frame's layout, the row pass
template <class F>
int gate_commit_run(const F& img, const int* idx, int n, unsigned char* key, long long* gstate, const float* focus, const long long* src_cat,
                    const long long* src_stats, const int* src_counts, const unsigned int* src_bits, const float* src_conf, long long* dst_cat,
                    long long* dst_stats, int* dst_counts, unsigned int* dst_bits, float* dst_conf, int B, int H, int W, int cap,
                    hipStream_t stream) {
  FS_REQUIRE(img && key && gstate && focus && B > 0 && H > 0 && W > 0 && (long)H * W < GATE_INT_LIMIT && n >= 0 && n <= B);
  FS_REQUIRE(H <= GATE_MAX_SIDE && W <= GATE_MAX_SIDE && cap >= 1 && img.ok(B, H, W));
  FS_REQUIRE(src_cat && src_stats && src_counts && src_bits && dst_cat && dst_stats && dst_counts && dst_bits);
  FS_REQUIRE((src_conf == nullptr) == (dst_conf == nullptr) && (n == 0 || idx != nullptr));
  const size_t per = (size_t)3 * H * W;
  const bool vec = img.wide_commit(W, per) && gate_key_ok<F>(key);
  const long bpi = (long)((per / (vec ? F::lane : 1) + GATE_THREADS - 1) / GATE_THREADS);
  GateRows r;
  const long nbits = (long)H * mask_row_words(W);
  const void* src[5] = {src_cat, src_stats, src_counts, src_bits, src_conf};
  void* dst[5] = {dst_cat, dst_stats, dst_counts, dst_bits, dst_conf};
  const long words[5] = {2, 12, cap, nbits, 3};
  long total = 0;
  for (int k = 0; k < 5; ++k) {
    const bool moves = src[k] != nullptr && src[k] != dst[k];
    r.src[k] = static_cast<const unsigned int*>(src[k]);
    r.dst[k] = static_cast<unsigned int*>(dst[k]);
    r.words[k] = moves ? (unsigned int)words[k] : 0u;
    total += moves ? words[k] : 0;
  }
  FS_REQUIRE(total < GATE_INT_LIMIT);
  r.total = (unsigned int)total;
  const long bpr = (total + GATE_THREADS - 1) / GATE_THREADS;
  FS_REQUIRE((long)n * bpi <= GATE_WGS_MAX && (long)n * bpr <= GATE_WGS_MAX);
  hipLaunchKernelGGL(gate_commit_state_kernel, dim3((unsigned)cdiv(B, GATE_THREADS)), dim3(GATE_THREADS), 0, stream, idx, n, gstate, focus, B, H, W);
  FS_LAUNCH_CHECK();
  if (n == 0) return FS_OK;
  gate_commit_frame(img, idx, key, B, H, W, per, vec, n * bpi, bpi, stream);
  FS_LAUNCH_CHECK();
  if (total > 0) {
    hipLaunchKernelGGL(gate_commit_rows_kernel, dim3((unsigned)(n * bpr)), dim3(GATE_THREADS), 0, stream, idx, B, r, (unsigned)bpr);
    FS_LAUNCH_CHECK();
  }
  return FS_OK;
}

}  // namespace

extern "C" {

int fs_gate_tiles(const float* img, const unsigned char* key, int* sad, int B, int H, int W, int T, hipStream_t stream) {
  FS_REQUIRE(img && key && sad && B > 0 && H > 0 && W > 0 && gate_tile_ok(T) && (long)H * W < GATE_INT_LIMIT);
  const int th = cdiv(H, T), tw = cdiv(W, T);
  const bool vec = PlanarFrame<float>(img, H, W).wide(W) && gate_key_ok<PlanarFrame<float>>(key);
  const int nseg = cdiv(W, GATE_SEG);
  const long wgs = (long)B * th * (vec ? nseg : tw);
  FS_REQUIRE((long)B * th * tw <= GATE_WGS_MAX);
  if (vec)
    hipLaunchKernelGGL(gate_tiles_band_kernel, dim3((unsigned)wgs), dim3(GATE_THREADS), 0, stream, img, key, sad, H, W, T, th, tw, nseg);
  else
    hipLaunchKernelGGL(gate_tiles_kernel, dim3((unsigned)wgs), dim3(GATE_THREADS), 0, stream, img, key, sad, H, W, T, th, tw);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

int fs_gate_tiles_u8(const unsigned char* img, const unsigned char* key, int* sad, int B, int H, int W, int T, hipStream_t stream) {
  return gate_tiles_bytes(PlanarFrame<unsigned char>(img, H, W), key, sad, B, H, W, T, stream);
}

int fs_gate_decide(const int* sad, const long long* gstate, const float* focus, const long long* stats, const unsigned int* bits,
                   const int* force, long long* gate, int B, int H, int W, int T, int level, int scene_tiles, int roi_tiles, int margin,
                   long saccade2, long fixation2, int max_age, int inside_on, hipStream_t stream) {
  FS_REQUIRE(sad && gstate && focus && stats && bits && gate && B > 0 && H > 0 && W > 0 && gate_tile_ok(T) && (long)H * W < GATE_INT_LIMIT);
  FS_REQUIRE(level >= 0 && level <= 254 && margin >= 0 && H <= GATE_MAX_SIDE && W <= GATE_MAX_SIDE && B <= GATE_WGS_MAX);
  GateRule p;
  p.H = H, p.W = W, p.T = T, p.th = cdiv(H, T), p.tw = cdiv(W, T), p.P = mask_row_words(W);
  p.level = level, p.scene_tiles = scene_tiles, p.roi_tiles = roi_tiles, p.margin = margin, p.max_age = max_age, p.inside_on = inside_on;
  p.saccade2 = saccade2, p.fixation2 = fixation2;
  hipLaunchKernelGGL(gate_decide_kernel, dim3((unsigned)B), dim3(GATE_THREADS), 0, stream, sad, gstate, focus, stats, bits, force, gate, p);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

int fs_gate_commit(const float* img, const int* idx, int n, unsigned char* key, long long* gstate, const float* focus,
                   const long long* src_cat, const long long* src_stats, const int* src_counts, const unsigned int* src_bits,
                   const float* src_conf, long long* dst_cat, long long* dst_stats, int* dst_counts, unsigned int* dst_bits, float* dst_conf,
                   int B, int H, int W, int cap, hipStream_t stream) {
  return gate_commit_run(PlanarFrame<float>(img, H, W), idx, n, key, gstate, focus, src_cat, src_stats, src_counts, src_bits, src_conf, dst_cat, dst_stats,
                         dst_counts, dst_bits, dst_conf, B, H, W, cap, stream);
}

int fs_gate_commit_u8(const unsigned char* img, const int* idx, int n, unsigned char* key, long long* gstate, const float* focus,
                      const long long* src_cat, const long long* src_stats, const int* src_counts, const unsigned int* src_bits,
                      const float* src_conf, long long* dst_cat, long long* dst_stats, int* dst_counts, unsigned int* dst_bits, float* dst_conf,
                      int B, int H, int W, int cap, hipStream_t stream) {
  return gate_commit_run(PlanarFrame<unsigned char>(img, H, W), idx, n, key, gstate, focus, src_cat, src_stats, src_counts, src_bits, src_conf, dst_cat,
                         dst_stats, dst_counts, dst_bits, dst_conf, B, H, W, cap, stream);
}

int fs_gate_tiles_hwc(const unsigned char* img, long sb, long sy, int sx, const unsigned char* key, int* sad, int B, int H, int W, int T,
                      hipStream_t stream) {
  return gate_tiles_bytes(HwcFrame<0>(img, sb, sy, sx), key, sad, B, H, W, T, stream);
}

int fs_gate_commit_hwc(const unsigned char* img, long sb, long sy, int sx, const int* idx, int n, unsigned char* key, long long* gstate,
                       const float* focus, const long long* src_cat, const long long* src_stats, const int* src_counts,
                       const unsigned int* src_bits, const float* src_conf, long long* dst_cat, long long* dst_stats, int* dst_counts,
                       unsigned int* dst_bits, float* dst_conf, int B, int H, int W, int cap, hipStream_t stream) {
  return gate_commit_run(HwcFrame<0>(img, sb, sy, sx), idx, n, key, gstate, focus, src_cat, src_stats, src_counts, src_bits, src_conf, dst_cat, dst_stats,
                         dst_counts, dst_bits, dst_conf, B, H, W, cap, stream);
}

int fs_gate_tiles_nv12(const unsigned char* yp, const unsigned char* uvp, long sb, long sy, long ub, long uy, int yo, int yg, int rv, int gu, int gv,
                       int bu, const unsigned char* key, int* sad, int B, int H, int W, int T, hipStream_t stream) {
  return gate_tiles_bytes(Nv12Frame(yp, uvp, sb, sy, ub, uy, Nv12Csc{yo, yg, rv, gu, gv, bu}), key, sad, B, H, W, T, stream);
}

int fs_gate_commit_nv12(const unsigned char* yp, const unsigned char* uvp, long sb, long sy, long ub, long uy, int yo, int yg, int rv, int gu, int gv,
                        int bu, const int* idx, int n, unsigned char* key, long long* gstate, const float* focus, const long long* src_cat,
                        const long long* src_stats, const int* src_counts, const unsigned int* src_bits, const float* src_conf, long long* dst_cat,
                        long long* dst_stats, int* dst_counts, unsigned int* dst_bits, float* dst_conf, int B, int H, int W, int cap,
                        hipStream_t stream) {
  return gate_commit_run(Nv12Frame(yp, uvp, sb, sy, ub, uy, Nv12Csc{yo, yg, rv, gu, gv, bu}), idx, n, key, gstate, focus, src_cat, src_stats, src_counts,
                         src_bits, src_conf, dst_cat, dst_stats, dst_counts, dst_bits, dst_conf, B, H, W, cap, stream);
}

}  // extern "C"
