// COCO / LVIS polygon lists into bit words (fs_poly_bits).  The reference makes its labels this way in its dataset preparation
// (DynamicFocus/e_preprocess_scripts/b2_preprocess_lvis.py:282-297: np.round, clip onto the frame, skimage.draw.polygon per polygon,
// the union as Y).  UNPINNED: skimage is not at hand, so the definition below is this library's, restated from that call site -- what
// skimage.draw.polygon is understood to give for integer vertices (interior plus edge and vertex points), not verified against it; it
// is NOT pycocotools' frPoly, which traces a 5x upsampled outline and differs along the rim.  DESIGN.md §1 f-3.
//   vertex  (vy, vx) = (clamp(y, 0, Hs-1), clamp(x, 0, Ws-1)) of the rounded (y, x) handed in: any int32 is defined, none is an address.
//   ring    the closed chain of a polygon's n >= 1 vertices, edges (v_i, v_(i+1) mod n).
//   pixel   (y, x) is set by a ring iff (a) it lies on an edge, end points included, or (b) the number of edges, oriented so that
//           y0 < y1, with y0 <= y < y1 and (x - x0)(y1 - y0) < (y - y0)(x1 - x0) is odd (even-odd; horizontal edges do not count).
//   mask    the OR of the image's rings: overlapping polygons do not cancel, a self-intersecting ring follows even-odd.
// All of it is integer work on bit words in LDS.  A workgroup owns one image and one band of `rows` rows (poly_plan) and keeps two row
// buffers, toggles and the accumulated mask.  Ring after ring:
//   edges   lanes stride over the ring's edges.  A non-horizontal edge walks its rows inside the band with an incremental exact
//           division (f, rem) = divmod((y - y0) dx, dy): rem == 0 is a lattice point of the edge, ORed into the mask; for y < y1 the
//           bit at c = x0 + ceil((y - y0) dx / dy) = x0 + f + (rem > 0) of the toggle row is flipped.  A row's crossings are even in
//           number, so "crossings right of x are odd" equals "toggles at or left of x are odd".  A horizontal edge ORs its span of word
//           masks.  c and every lattice point lie between the edge's two clamped ends, hence inside the row.
//   scan    the inclusive prefix-XOR along each toggled row: five shift-XORs inside a word, the parity of the words before it from a
//           ballot over the wave; the result is ORed into the mask and the toggle word cleared for the next ring.
// After the last ring the band is stored, every word by a plain store, and its popcount goes to scratch; a second kernel adds an
// image's bands into info.  XOR and OR in LDS do not depend on order: the same bits in every mode and in every run.
#include "mask_words.h"

namespace {

constexpr int POLY_THREADS = 256;
constexpr int POLY_WAVES = POLY_THREADS / 64;
constexpr int POLY_BAND_ROWS = 64;                     // rows a band at the most
constexpr int POLY_BAND_WORDS = 4096;                  // words a row buffer at the most: two buffers are 32 KiB of LDS

struct PolyPlan {
  int P, rows, bands;                                  // words a row; rows a band; bands an image
  long parts;                                          // scratch, in ints: the popcount of every (image, band)
  bool ok;
};

PolyPlan poly_plan(int B, int Hs, int Ws) {
  PolyPlan p = {};
  if (!(B > 0 && Hs > 0 && Ws > 0 && Hs <= MASK_MAX_SIDE && Ws <= MASK_MAX_SIDE)) return p;     // (y - y0) dx stays below 2^28
  p.P = mask_row_words(Ws);
  // Bands of 64 rows (32 KiB of LDS at the most) were measured against bands that fill 64 KiB (250 rows at 1024 wide) on one MI355X at
  // B = 64: the tall bands were 1.35 - 1.94 x slower on every case of tools/poly_bench.py (a quarter of the workgroups, each clearing,
  // scanning and storing four times the rows), 128 rows 1.08 - 1.25 x slower on four of five, 16 rows 0 - 7 % slower
  // (profiles/r30/README.md).  FS_POLY_BAND / FS_POLY_WORDS exist in kernel A/B builds only (words <= 8000).
  static const int band_rows = FS_ENV_INT("FS_POLY_BAND", POLY_BAND_ROWS), band_words = FS_ENV_INT("FS_POLY_WORDS", POLY_BAND_WORDS);
  const int fit = band_words / p.P;                    // >= 8: P <= 512
  p.rows = min(Hs, min(band_rows, fit));
  p.bands = cdiv(Hs, p.rows);
  p.parts = (long)B * p.bands;
  // a workgroup stores at least one row, so the grid stays below 2^31 with the slots below 2^32
  p.ok = (long)Hs * Ws < MASK_INT_LIMIT && (long)B * Hs * p.P * 32 <= THREADS_MAX;     // bit slots, as fs_mask_bits
  return p;
}

__device__ __forceinline__ int poly_clamp(int v, int top) { return v < 0 ? 0 : (v > top ? top : v); }

__device__ __forceinline__ unsigned int poly_prefix_xor(unsigned int w) {              // bit j = the parity of bits 0 .. j
  w ^= w << 1, w ^= w << 2, w ^= w << 4, w ^= w << 8, w ^= w << 16;
  return w;
}

// grid = B * bands; dynamic LDS = 2 * rows * P words (toggles, mask).  SKIP is 0 in the shipped library; kernel A/B builds time the
// phases by leaving one out: 1 no scan, 2 no edge pass either (what is left clears, stores and counts).
template <int SKIP>
__global__ __launch_bounds__(POLY_THREADS) void poly_band_kernel(const int* __restrict__ verts, const int* __restrict__ ring_off,
                                                                 const int* __restrict__ img_ring, unsigned int* __restrict__ bits,
                                                                 long long* __restrict__ info, int* __restrict__ parts, int R, int V, int Hs,
                                                                 int Ws, int P, int rows, int bands) {
  extern __shared__ unsigned int poly_lds[];
  __shared__ int span[2][2];                           // (first, last) toggled row of a ring, by the ring's parity
  __shared__ int wcnt[POLY_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int img = blockIdx.x / bands, band = blockIdx.x - img * bands;
  const int r0 = band * rows, r1 = min(r0 + rows, Hs), nr = r1 - r0, nw = nr * P;
  unsigned int* tog = poly_lds;
  unsigned int* acc = poly_lds + rows * P;
  for (int i = tid; i < nw; i += POLY_THREADS) tog[i] = 0u, acc[i] = 0u;
  if (tid < 2) span[tid][0] = nr, span[tid][1] = -1;

  const int ra = img_ring[img], rb = img_ring[img + 1];
  int bad = !(0 <= ra && ra <= rb && rb <= R);
  if (!bad) {
    for (int r = ra + tid; r < rb; r += POLY_THREADS) {                               // r + 1 <= rb <= R: inside ring_off
      const int a = ring_off[r], b = ring_off[r + 1];
      bad |= !(0 <= a && a <= b && b <= V);
    }
  }
  bad = __syncthreads_or(bad);                         // the workgroup's; the buffers are clear behind it

  if (!bad) {
    // the scan's lane layout: with P <= 64 a wave takes 64 / P whole rows at once, lane <-> (row lr, word lc); else a row in chunks
    const int rpw = P <= 64 ? 64 / P : 1;
    const int lr = P <= 64 ? lane / P : 0, lc = lane - lr * P;
    int k = 0;                                         // rings with vertices so far
    for (int r = ra; r < rb; ++r) {                    // uniform
      const int v0 = ring_off[r], n = ring_off[r + 1] - v0;
      if (n == 0) continue;
      const int s = k & 1;
      ++k;
      int lo = nr, hi = -1;
      for (int e = tid; e < (SKIP & 2 ? 0 : n); e += POLY_THREADS) {
        const size_t i0 = (size_t)v0 + e, i1 = (size_t)v0 + (e + 1 == n ? 0 : e + 1);
        int ya = poly_clamp(verts[2 * i0], Hs - 1), xa = poly_clamp(verts[2 * i0 + 1], Ws - 1);
        int yb = poly_clamp(verts[2 * i1], Hs - 1), xb = poly_clamp(verts[2 * i1 + 1], Ws - 1);
        if (ya == yb) {                                // horizontal, or a point: its span of the row
          if (ya >= r0 && ya < r1) {
            const int xl = min(xa, xb), xr = max(xa, xb);
            unsigned int* row = acc + (ya - r0) * P;
            for (int w = xl >> 5; w <= xr >> 5; ++w) {
              unsigned int m = ~0u;
              if (w == xl >> 5) m &= ~0u << (xl & 31);
              if (w == xr >> 5) m &= ~0u >> (31 - (xr & 31));
              atomicOr(&row[w], m);
            }
          }
          continue;
        }
        if (ya > yb) {
          int t = ya; ya = yb, yb = t;
          t = xa, xa = xb, xb = t;
        }
        const int ys = max(ya, r0), ye = min(yb, r1 - 1);
        if (ys > ye) continue;
        const int dy = yb - ya, dx = xb - xa;
        const int num = (ys - ya) * dx;                // |num| < 2^28
        int f = num / dy, rem = num - f * dy;
        if (rem < 0) rem += dy, --f;                   // floor
        int qs = dx / dy, rs = dx - qs * dy;
        if (rs < 0) rs += dy, --qs;
        for (int y = ys; y <= ye; ++y) {
          const int x = xa + f;
          unsigned int* row = (y - r0) * P + acc;
          if (rem == 0) atomicOr(&row[x >> 5], 1u << (x & 31));
          if (y < yb) {
            const int c = x + (rem > 0);
            atomicXor(&tog[(y - r0) * P + (c >> 5)], 1u << (c & 31));
          }
          f += qs, rem += rs;
          if (rem >= dy) rem -= dy, ++f;
        }
        const int te = min(ye, yb - 1);
        if (ys <= te) lo = min(lo, ys - r0), hi = max(hi, te - r0);
      }
      if (hi >= 0) atomicMin(&span[s][0], lo), atomicMax(&span[s][1], hi);
      __syncthreads();
      const int slo = span[s][0], shi = span[s][1];
      if (tid == 0) span[s ^ 1][0] = nr, span[s ^ 1][1] = -1;                          // the next ring's; last read before the barrier above
      if (SKIP & 1) {
      } else if (P <= 64) {
        for (int g = slo + wave * rpw; g <= shi; g += POLY_WAVES * rpw) {               // the wave's
          const int row = g + lr;
          const bool live = lr < rpw && row <= shi;
          const int at = row * P + lc;
          const unsigned int w = poly_prefix_xor(live ? tog[at] : 0u);
          const unsigned long long odd = __ballot(w >> 31);
          const unsigned long long before = ((1ull << lc) - 1ull) << (lane - lc);      // the words of this row left of this one
          if (live) {
            acc[at] |= (__popcll(odd & before) & 1) ? ~w : w;
            tog[at] = 0u;
          }
        }
      } else {
        for (int row = slo + wave; row <= shi; row += POLY_WAVES) {
          int carry = 0;
          for (int c0 = 0; c0 < P; c0 += 64) {
            const bool live = c0 + lane < P;
            const int at = row * P + c0 + lane;
            const unsigned int w = poly_prefix_xor(live ? tog[at] : 0u);
            const unsigned long long odd = __ballot(w >> 31);
            if (live) {
              acc[at] |= ((carry + __popcll(odd & ((1ull << lane) - 1ull))) & 1) ? ~w : w;
              tog[at] = 0u;
            }
            carry ^= __popcll(odd) & 1;
          }
        }
      }
      __syncthreads();
    }
  }

  int cnt = 0;
  unsigned int* dst = bits + ((size_t)img * Hs + r0) * P;
  for (int i = tid; i < nw; i += POLY_THREADS) {
    const unsigned int w = bad ? 0u : acc[i];
    dst[i] = w;
    cnt += __popc(w);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if (lane == 0) wcnt[wave] = cnt;
  __syncthreads();
  if (tid == 0) {
    int all = 0;
    for (int w = 0; w < POLY_WAVES; ++w) all += wcnt[w];
    parts[blockIdx.x] = all;                           // at most 64 * 16384 set pixels a band
    if (band == 0) {
      info[(size_t)img * 4 + 0] = bad ? 1 : 0;
      info[(size_t)img * 4 + 2] = bad ? 0 : rb - ra;
      info[(size_t)img * 4 + 3] = bad || rb == ra ? 0 : ring_off[rb] - ring_off[ra];
    }
  }
}

// grid = B, one wave: info[b].area = the sum of the image's bands
__global__ __launch_bounds__(64) void poly_area_kernel(const int* __restrict__ parts, long long* __restrict__ info, int bands) {
  const size_t img = blockIdx.x;
  long long sum = 0;
  for (int i = threadIdx.x; i < bands; i += 64) sum += parts[img * bands + i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  if (threadIdx.x == 0) info[img * 4 + 1] = sum;
}

}  // namespace

extern "C" {

long fs_poly_bits_scratch_ints(int B, int Hs, int Ws) { return poly_plan(B, Hs, Ws).parts; }

int fs_poly_bits_band_rows(int Hs, int Ws) { return poly_plan(1, Hs, Ws).rows; }

int fs_poly_bits(const int* verts, const int* ring_off, const int* img_ring, unsigned int* bits, long long* info, int* scratch, int B, int R,
                 int V, int Hs, int Ws, hipStream_t stream) {
  const PolyPlan p = poly_plan(B, Hs, Ws);
  FS_REQUIRE(verts && ring_off && img_ring && bits && info && scratch && R >= 0 && V >= 0 && p.ok);
  const size_t lds = 2 * (size_t)p.rows * p.P * sizeof(unsigned int);
#ifdef FS_EXPERIMENTS
  static const int skip = FS_ENV_INT("FS_POLY_SKIP", 0);
  if (skip == 1)
    hipLaunchKernelGGL(poly_band_kernel<1>, dim3((unsigned)p.parts), dim3(POLY_THREADS), lds, stream, verts, ring_off, img_ring, bits, info,
                       scratch, R, V, Hs, Ws, p.P, p.rows, p.bands);
  else if (skip == 3)
    hipLaunchKernelGGL(poly_band_kernel<3>, dim3((unsigned)p.parts), dim3(POLY_THREADS), lds, stream, verts, ring_off, img_ring, bits, info,
                       scratch, R, V, Hs, Ws, p.P, p.rows, p.bands);
  else
#endif
  hipLaunchKernelGGL(poly_band_kernel<0>, dim3((unsigned)p.parts), dim3(POLY_THREADS), lds, stream, verts, ring_off, img_ring, bits, info,
                     scratch, R, V, Hs, Ws, p.P, p.rows, p.bands);
  FS_LAUNCH_CHECK();
  hipLaunchKernelGGL(poly_area_kernel, dim3((unsigned)B), dim3(64), 0, stream, (const int*)scratch, info, p.bands);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

}  // extern "C"
