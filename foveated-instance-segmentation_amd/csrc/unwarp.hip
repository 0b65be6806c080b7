// The inverse (un-foveating) warp and the full-resolution evaluation built on it (gather bound).  Stages:
//   index maps   trunc-toward-zero integer maps of the inverse deformation                  (models/models.py:644-645)
//   owner        every grid point claims the full-resolution pixel it was sampled from; the last claim wins; the inverse grid
//                                                                                            (models/models.py:639-655,931-932)
//   fill         exact nearest claimed pixel for the holes: nearest column per row, then the best row   (models.py:159-286, 'nearest')
//   decide       the C1 head's argmax once per grid point, gathered through owner + fill -> class map    (models/models.py:930-940; eval.py:195)
//   gather       which grid point feeds a full-resolution pixel: feeding_point / feeding_points4, the one rule under every stage below;
//                its bit-word output: gather_bits over mask_words.h's bit_slot, store_word_nibbles / store_word_ballot
//   count        the same gather, counting against the label instead of storing: the six counters and four accuracies of
//                MODEL.upsample (models/models.py:378-474,968), the trimap buckets (eval.py:41-67), the per-class areas of the three
//                spaces (eval.py:197,218-257,313-322; models/models_instance.py:909-918; utils.py:289-317)
//   trimap bands which band of width 1, 2, 4 .. 2^D around the label's boundary a pixel lies in     (eval.py:41-67)
//   surface      the q-th percentile of the distances between two masks' borders (HD95), as two integer order statistics of d^2
//                                                                                            (VAL.hd95; utils.py:25-101, in 2-D)
//   instance     the mask "class is not K-1" gathered into bit words, its area, box and uncompressed COCO run-length code (mask_rle.hip's
//                passes), and the head's class: the label-free output as a record (no counterpart in the reference)
//   score        the record's confidence: the foreground softmax mass per grid point as a 24-bit integer table, summed over the set pixels
//                in the instance gather, times the head's class probability (no counterpart in the reference; unpinned)
// Host side: fs_unwarp_labels / _accuracy / _trimap / _class_areas / _hd / _instances / _instances_scored / _instances_component are one
// launch sequence with optional parts.  unwarp_plan() derives
// every size, scratch offset and limit from the shape and the feature set, UnwarpJob carries the caller's pointers, unwarp_run()
// checks both and launches.  A refused call launches nothing: every check, fs_trimap_bands' included, comes before the first launch.
#include "mask_words.h"
#include "grid_taps.h"

namespace {

// integer index maps of the inverse deformation (models/models.py:644-645): trunc toward zero
__global__ void inverse_index_kernel(const float* __restrict__ grid, long long* __restrict__ u, long long* __restrict__ v,
                                     long n, int H, int W) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float gx = grid[2 * i], gy = grid[2 * i + 1];
  const float fu = __fmul_rn(__fmul_rn(__fadd_rn(gx, 1.f), 0.5f), (float)(W - 1));
  const float fv = __fmul_rn(__fmul_rn(__fadd_rn(gy, 1.f), 0.5f), (float)(H - 1));
  u[i] = (long long)(int)fu;
  v[i] = (long long)(int)fv;
}

// ---- inverse (un-foveating) warp, SURVEY §8(f)-3 -------------------------------------------------------------------
// models/models.py:639-655: every grid point i = (yi, xi) of the (h,w) sampling grid claims the full-resolution pixel
// (v,u) it was sampled from; duplicate claims resolve as ATen-CPU index_put_ does (the LAST index wins = largest i).
__global__ void inverse_owner_kernel(const float* __restrict__ grid, int* __restrict__ owner, int B, int hw, int Hs, int Ws) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)B * hw) return;
  const int b = (int)(i / hw), p = (int)(i - (long)b * hw);
  const float gx = grid[2 * i], gy = grid[2 * i + 1];
  const int u = (int)__fmul_rn(__fmul_rn(__fadd_rn(gx, 1.f), 0.5f), (float)(Ws - 1));
  const int v = (int)__fmul_rn(__fmul_rn(__fadd_rn(gy, 1.f), 0.5f), (float)(Hs - 1));
  if (u < 0 || u >= Ws || v < 0 || v >= Hs) return;
  atomicMax(&owner[((long)b * Hs + v) * Ws + u], p);
}
// grid_inv[b,v,u] = (xi/w*2-1, yi/h*2-1) of the owning grid point, 0 where nobody claims the pixel (the reference writes NaN
// and replaces it by 0 before sampling, models.py:931-932; the hole mask is owner < 0).
__global__ void inverse_grid_kernel(const int* __restrict__ owner, float* __restrict__ inv, long n, int h, int w) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int p = owner[i];
  float gx = 0.f, gy = 0.f;
  if (p >= 0) {
    const int yi = p / w, xi = p - yi * w;
    gx = __fsub_rn(__fmul_rn(__fdiv_rn((float)xi, (float)w), 2.f), 1.f);
    gy = __fsub_rn(__fmul_rn(__fdiv_rn((float)yi, (float)h), 2.f), 1.f);
  }
  inv[2 * i] = gx; inv[2 * i + 1] = gy;
}
// Nearest-valid fill (models.py:159-286 with rev_deform_interp='nearest'): exact Euclidean nearest claimed pixel, ties to
// the smallest (row, col).  Pass A: nearest claimed column in the same row; pass B: minimise (y-y')^2 + (x-x'(y'))^2 over rows.
__global__ __launch_bounds__(256) void fill_row_nearest_kernel(const int* __restrict__ owner, int* __restrict__ rowx, int Ws) {
  extern __shared__ int rowbuf[];                      // [Ws]: claimed flag, then nearest claimed column
  __shared__ int carryL[256], carryR[256];
  const int tid = threadIdx.x;
  const long row = blockIdx.x;
  const int* o = owner + row * Ws;
  int* r = rowx + row * Ws;
  int any = 0;
  for (int x = tid; x < Ws; x += 256) { const int c = o[x] >= 0; rowbuf[x] = c; any |= c; }
  // most rows of a strongly magnified image hold no claimed pixel at all
  if (!__syncthreads_or(any)) {
    for (int x = tid; x < Ws; x += 256) r[x] = -1;
    return;
  }
  // thread t owns the columns [x0, x1): last / first claimed column of the segment, then a scan over the 256 segments
  const int seg = (Ws + 255) / 256;
  const int x0 = tid * seg < Ws ? tid * seg : Ws, x1 = x0 + seg < Ws ? x0 + seg : Ws;
  int last = -1, first = 0x7fffffff;
  for (int x = x0; x < x1; ++x)
    if (rowbuf[x]) { last = x; if (first == 0x7fffffff) first = x; }
  carryL[tid] = last; carryR[tid] = first;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    int l = carryL[tid], rr = carryR[tid];
    if (tid >= off) { const int v = carryL[tid - off]; l = v > l ? v : l; }
    if (tid + off < 256) { const int v = carryR[tid + off]; rr = v < rr ? v : rr; }
    __syncthreads();
    carryL[tid] = l; carryR[tid] = rr;
    __syncthreads();
  }
  int left = tid > 0 ? carryL[tid - 1] : -1;
  int right = tid < 255 ? carryR[tid + 1] : 0x7fffffff;
  for (int x = x0; x < x1; ++x) {                      // nearest claimed column at or left of x
    if (rowbuf[x]) left = x;
    rowbuf[x] = left;
  }
  for (int x = x1 - 1; x >= x0; --x) {                 // ... against the nearest at or right of x; a tie goes to the left one
    const int l = rowbuf[x];
    if (l == x) right = x;
    int best;
    if (l < 0) best = right == 0x7fffffff ? -1 : right;
    else if (right == 0x7fffffff) best = l;
    else best = (x - l) <= (right - x) ? l : right;
    rowbuf[x] = best;
  }
  __syncthreads();
  for (int x = tid; x < Ws; x += 256) r[x] = rowbuf[x];
}
// pixel index y'*Ws+x' of the claimed pixel nearest to (y, x), -1 when the image has none; rx = the image's rows of fill_row_nearest_kernel
__device__ __forceinline__ int nearest_claimed(const int* __restrict__ rx, int y, int x, int Hs, int Ws) {
  long best = -1;
  int bsrc = -1;
  for (int d = 0; d < Hs; ++d) {                       // rows by increasing |y - y'|: stop once dy^2 alone exceeds the best
    if (best >= 0 && (long)d * d > best) break;
    for (int sgn = 0; sgn < 2; ++sgn) {
      const int yy = sgn == 0 ? y - d : y + d;
      if (yy < 0 || yy >= Hs || (d == 0 && sgn == 1)) continue;
      const int xx = rx[(long)yy * Ws + x];
      if (xx < 0) continue;
      const long dd = (long)d * d + (long)(x - xx) * (x - xx);
      const int cand = yy * Ws + xx;
      if (best < 0 || dd < best || (dd == best && cand < bsrc)) { best = dd; bsrc = cand; }
    }
  }
  return bsrc;
}
// nearest_claimed for the four pixels (y, x .. x+3) of one row at once (x % 4 == 0, Ws % 4 == 0): one 16-byte read of rx per row serves
// all four.  Every pixel sees its candidates in nearest_claimed's order and under its comparison; the rows past the point where
// nearest_claimed would have stopped for it cannot win (dd >= d*d > best), so each src[k] is nearest_claimed's.  A claimed pixel
// (hole bit clear) takes no part.
__device__ __forceinline__ void nearest_claimed4(const int* __restrict__ rx, int y, int x, int Hs, int Ws, int holes, int src[4]) {
  long best[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) { best[k] = (holes >> k) & 1 ? -1 : 0; src[k] = -1; }
  for (int d = 0; d < Hs; ++d) {
    const long d2 = (long)d * d;
    bool done = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) done = done && best[k] >= 0 && d2 > best[k];
    if (done) break;
    for (int sgn = 0; sgn < 2; ++sgn) {
      const int yy = sgn == 0 ? y - d : y + d;
      if (yy < 0 || yy >= Hs || (d == 0 && sgn == 1)) continue;
      const int4 r = *reinterpret_cast<const int4*>(rx + (long)yy * Ws + x);
      const int xs[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int xx = xs[k];
        if (xx < 0) continue;
        const long dx = (long)(x + k - xx);
        const long dd = d2 + dx * dx;
        const int cand = yy * Ws + xx;
        if (best[k] < 0 || dd < best[k] || (dd == best[k] && cand < src[k])) { best[k] = dd; src[k] = cand; }
      }
    }
  }
}
// THE rule of every full-resolution result: the grid point that feeds pixel (y, x) of an image is the pixel's owner o; for a hole
// (o < 0) the owner of the nearest claimed pixel; point hw = h*w, the sample at (0,0), in an image without any claim.  ob, rx = the
// image's owner map and its rows of fill_row_nearest_kernel.  Every table read through the result has hw + 1 entries an image.
__device__ __forceinline__ int feeding_point(const int* __restrict__ ob, const int* __restrict__ rx, int o, int y, int x, int Hs, int Ws,
                                             int hw) {
  if (o >= 0) return o;
  const int src = nearest_claimed(rx, y, x, Hs, Ws);
  return src >= 0 ? ob[src] : hw;
}
// the same for the four pixels (y, x .. x+3), x % 4 == 0, Ws % 4 == 0, ob and rx 16-byte aligned: one 16-byte read of their owners
__device__ __forceinline__ void feeding_points4(const int* __restrict__ ob, const int* __restrict__ rx, int y, int x, int Hs, int Ws, int hw,
                                                int q[4]) {
  const int4 o4 = *reinterpret_cast<const int4*>(ob + y * Ws + x);
  q[0] = o4.x; q[1] = o4.y; q[2] = o4.z; q[3] = o4.w;
  const int holes = (o4.x < 0) | (o4.y < 0) << 1 | (o4.z < 0) << 2 | (o4.w < 0) << 3;
  if (holes) {
    int src[4];
    nearest_claimed4(rx, y, x, Hs, Ws, holes, src);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if ((holes >> k) & 1) q[k] = src[k] >= 0 ? ob[src[k]] : hw;
  }
}
__global__ void fill_col_nearest_kernel(const int* __restrict__ rowx, int* __restrict__ src, long n, int Hs, int Ws) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const long per = (long)Hs * Ws;
  const long b = i / per;
  const long rem = i - b * per;
  const int y = (int)(rem / Ws), x = (int)(rem - (long)y * Ws);
  src[i] = nearest_claimed(rowx + b * per, y, x, Hs, Ws);
}
__global__ void fill_copy_kernel(float* __restrict__ vals, const int* __restrict__ owner, const int* __restrict__ src, int C, long per,
                                 long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;       // over (b, pixel): the source index is looked up once for all classes
  if (i >= n) return;
  if (owner[i] >= 0) return;                           // claimed pixels keep their sampled value
  const int sp = src[i];
  if (sp < 0) return;                                  // image without any claimed pixel
  const long b = i / per;
  const long pix = i - b * per;
  float* v = vals + b * C * per;
  int c = 0;
  for (; c + 4 <= C; c += 4) {                          // four independent gathers in flight per trip
    const float a0 = v[(c + 0) * per + sp], a1 = v[(c + 1) * per + sp], a2 = v[(c + 2) * per + sp], a3 = v[(c + 3) * per + sp];
    v[(c + 0) * per + pix] = a0; v[(c + 1) * per + pix] = a1; v[(c + 2) * per + pix] = a2; v[(c + 3) * per + pix] = a3;
  }
  for (; c < C; ++c) v[c * per + pix] = v[c * per + sp];
}

// ---- class map at full resolution without the (B,K,Hs,Ws) prediction ----------------------------------------------------------------
// The C1 prediction is pred[b,k] = cls[b,k] (k < K-1, one constant plane) and pred[b,K-1] = cls[b,K-1] * m[b] (fs_pred_assemble_fwd).
// Through the inverse warp every full-resolution pixel carries the sample of pred at ONE grid point's inverse coordinate: its owner's
// if claimed, its nearest claimed pixel's owner's if a hole, (0,0) in an image without any claim.  So argmax_k of unwarp_nearest(pred)
// is a per-grid-point decision gathered through the owner map; both kernels repeat the float operations of the unfused route exactly.
constexpr int UNWARP_MAX_K = 1024;
// dec[b,p] = argmax_k of grid_sample(pred[b], inverse coordinate of point p) for p < h*w, and of the sample at (0,0) for p = h*w
__global__ __launch_bounds__(256) void unwarp_decide_kernel(const float* __restrict__ cls, const float* __restrict__ m, int* __restrict__ dec,
                                                            int K, int h, int w, int blocks_per_image) {
  __shared__ float cs[UNWARP_MAX_K];
  const int b = blockIdx.x / blocks_per_image;
  const int hw = h * w;
  for (int k = threadIdx.x; k < K; k += 256) cs[k] = cls[(long)b * K + k];
  __syncthreads();
  const int p = (blockIdx.x - b * blocks_per_image) * 256 + threadIdx.x;
  if (p > hw) return;
  float gx = 0.f, gy = 0.f;                            // the coordinate inverse_grid_kernel writes for this point / for a hole
  if (p < hw) {
    const int yi = p / w, xi = p - yi * w;
    gx = __fsub_rn(__fmul_rn(__fdiv_rn((float)xi, (float)w), 2.f), 1.f);
    gy = __fsub_rn(__fmul_rn(__fdiv_rn((float)yi, (float)h), 2.f), 1.f);
  }
  const Taps t = make_taps(gx, gy, h, w);
  const bool inw = t.oky0 & t.okx0, ine = t.oky0 & t.okx1, isw = t.oky1 & t.okx0, ise = t.oky1 & t.okx1;
  // sample_plane's sequence; a constant plane reads c at every in-bounds tap, 0 outside
  auto sample4 = [&](float vnw, float vne, float vsw, float vse) {
    float acc = __fmul_rn(vnw, t.nw);
    acc = __fmaf_rn(vne, t.ne, acc);
    acc = __fmaf_rn(vsw, t.sw, acc);
    return __fmaf_rn(vse, t.se, acc);
  };
  // torch.argmax: the first maximal index; NaN counts as the maximum
  float best = 0.f;
  int arg = 0;
  for (int k = 0; k < K - 1; ++k) {
    const float c = cs[k];
    const float v = sample4(inw ? c : 0.f, ine ? c : 0.f, isw ? c : 0.f, ise ? c : 0.f);
    if (k == 0 || v > best || (v != v && best == best)) { best = v; arg = k; }
  }
  const float c = cs[K - 1];
  const float* mp = m + (long)b * hw;
  const float v = sample4(inw ? __fmul_rn(c, mp[t.y0 * w + t.x0]) : 0.f, ine ? __fmul_rn(c, mp[t.y0 * w + t.x0 + 1]) : 0.f,
                          isw ? __fmul_rn(c, mp[(t.y0 + 1) * w + t.x0]) : 0.f, ise ? __fmul_rn(c, mp[(t.y0 + 1) * w + t.x0 + 1]) : 0.f);
  if (v > best || (v != v && best == best)) arg = K - 1;
  dec[(long)b * (hw + 1) + p] = arg;
}
// labels[b,v,u] = dec[b, feeding_point of the pixel]; hole (nullable) = the pixel has no owner.
__global__ __launch_bounds__(256) void unwarp_label_kernel(const int* __restrict__ owner, const int* __restrict__ rowx, const int* __restrict__ dec,
                                                           long long* __restrict__ labels, unsigned char* __restrict__ hole, long n, int Hs, int Ws,
                                                           int hw) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const long per = (long)Hs * Ws;
  const long b = i / per;
  const int rem = (int)(i - b * per);                  // per < 2^31
  const int y = rem / Ws, x = rem - y * Ws;
  const int o = owner[i];
  labels[i] = (long long)dec[b * (hw + 1) + feeding_point(owner + b * per, rowx + b * per, o, y, x, Hs, Ws, hw)];
  if (hole != nullptr) hole[i] = o < 0;
}

// ---- the four full-resolution accuracies without the class map ---------------------------------------------------------------------
// The gather with the compare-and-count of seg_loss_fwd_kernel behind it: the predicted class of a pixel is dec[its feeding_point],
// its ground truth one read of the label mask (t = (long)y, gt = t*cls_label + (1-t)*(K-1), models.py:968),
// and the six counters of models/models.py:378-474 are summed where the class would have been stored.
// pixels per thread: one trip of four neighbours.  8 and 16 (fewer records) measured slower: 614 / 616 against 519 us at B = 64, 1024^2,
// and 24 / 34 against 14 us at B = 1, where 256 workgroups a trip longer leave the CUs short of waves (profiles/r07)
constexpr int UACC_PIX = 4;
constexpr int UACC_CHUNK = 256 * UACC_PIX;             // pixels per workgroup, all of one image
constexpr int UACC_REC = 8;                            // ints per workgroup record: the six counters + 2 of padding (two 16-byte stores)
struct AccCount { int c[6]; };
// head_loss.hip's predicates (seg_loss_fwd_kernel) on one pixel: a = predicted class, yv = the label mask's value
__device__ __forceinline__ void count_pixel(AccCount& n, int a, float yv, long long cl, int bg) {
  const long long t = (long long)yv;
  const long long g = t * cl + (1 - t) * (long long)bg;
  const bool vg = g < bg, vp = a < bg, bgg = g == bg, bgp = a == bg, eq = (long long)a == g;
  n.c[0] += (vg && eq); n.c[1] += (vg && (vg == vp)); n.c[2] += (vg || vp);
  n.c[3] += (bgg && eq); n.c[4] += (bgg && (bgg == bgp)); n.c[5] += (bgg || bgp);
}
// grid = B * blocks_per_image workgroups; workgroup (b, chunk) counts UACC_CHUNK consecutive pixels of image b into ONE record of
// rec (plain stores: no zero-initialised scratch, no global atomics).  VEC: Ws % 4 == 0 and 16-byte aligned owner / y / labels, so
// that four neighbours are one row's and load as one dwordx4 each.  labels (nullable) receives unwarp_label_kernel's class map.
// TRIM (fs_unwarp_trimap): the pixel's band byte (fs_trimap_bands) buckets three more predicates -- in a band, class right, foreground /
// background right -- into trec; without it the body is fs_unwarp_accuracy's count pass as it was.
constexpr int TRIM_BUCKETS = 8;                        // band indices 0 .. D, D <= 7
constexpr int TRIM_REC = TRIM_BUCKETS * 3;             // ints per workgroup record: (total, cls_ok, bin_ok) per bucket, six 16-byte rows
// one LDS add per banded pixel: three 10-bit fields of its wave's bucket word (a wave counts at most 256 pixels)
__device__ __forceinline__ void trim_pixel(unsigned int* __restrict__ tbw, unsigned int bi, int a, float yv, long long cl, int bg) {
  if (bi >= (unsigned int)TRIM_BUCKETS) return;        // 255: in no band
  const long long t = (long long)yv;
  const long long g = t * cl + (1 - t) * (long long)bg;
  const unsigned int eq = (long long)a == g, bin = (a == bg) == (g == bg);
  atomicAdd(tbw + bi, 1u | eq << 10 | bin << 20);
}
// AREA (fs_unwarp_class_areas): the per-class areas of utils.intersectionAndUnion (utils.py:289-317) for two class maps against the
// ground truth g of count_pixel -- the predicted class a = dec[q] of the feeding point q, and the CEILING class a' = gs[q], gs[p] =
// ts[p]*cl + (1 - ts[p])*(K-1) with ts[p] grid_sample_label_kernel's value of point p bit for bit (the training label of that point;
// background for the point h*w of an image without any claim).  This is the reference's VAL.y_sampled_reverse, "intrinsic upsampling
// error IoU(Y', Y)" (models/models_instance.py:909-918, eval.py:220-244): the label after the sampler and the nearest un-warp, scored
// against itself.  The ceiling is the label of the feeding point ITSELF, not the reference's F.grid_sample(mode='nearest') at the
// inverse coordinate: that coordinate is xi - 0.5 up to fp32 rounding, so the reference's value is a round-half-to-even tie decided
// by rounding noise between the point and its left / upper neighbour.
// ts rides in bit DEC_TS_BIT of dec, set by class_area_sampled_kernel after unwarp_decide_kernel and masked in the AREA instantiations
// only; the others never see it (their launcher does not run that kernel) and stay the instruction streams they were.
// g and a' are cl or K-1, and almost every a is: those two HOT classes are counted in registers -- eight predicates in three words of
// 10-bit fields, a thread adding at most four pixels and a wave 256 -- reduced by shuffles and LDS into one AREA_REC-int record per
// workgroup (arec, two 16-byte stores).  A predicted class other than the two goes to a per-workgroup LDS histogram of K bins (zeroed
// at entry), whose non-zero bins are added with 32-bit integer global atomics into atab (B, K), zeroed by the launcher: atab holds
// SUMS, not records.  A workgroup without such a pixel (the usual case) skips the flush.  Integer sums: the same bits in any order.
constexpr int DEC_TS_BIT = 30;
constexpr int DEC_CLASS_MASK = (1 << DEC_TS_BIT) - 1;
constexpr int AREA_REC = 8;                            // t, a==cl & t, a==bg & !t | a==cl (not bg), a==bg, ts | ts & t, !ts & !t
struct AreaWords { unsigned int w[3]; unsigned int cold; };
// d = dec word of the feeding point (class | ts << DEC_TS_BIT); returns the class
__device__ __forceinline__ int area_pixel(AreaWords& r, int* __restrict__ hist, int d, float yv, long long cl, int bg) {
  const int a = d & DEC_CLASS_MASK;
  const unsigned int ts = (unsigned int)d >> DEC_TS_BIT;
  const unsigned int t = (long long)yv != 0;
  const unsigned int acl = (long long)a == cl, abg = a == bg;
  r.w[0] += t | (acl & t) << 10 | (abg & (t ^ 1u)) << 20;
  r.w[1] += (acl & (abg ^ 1u)) | abg << 10 | ts << 20;
  r.w[2] += (ts & t) | ((ts | t) ^ 1u) << 10;
  if (!(acl | abg)) { atomicAdd(hist + a, 1); r.cold = 1u; }
  return a;
}
template <bool VEC, bool TRIM, bool AREA>
__global__ __launch_bounds__(256) void unwarp_count_kernel(const int* __restrict__ owner, const int* __restrict__ rowx, const int* __restrict__ dec,
                                                           const float* __restrict__ yl, const long long* __restrict__ cls_label,
                                                           long long* __restrict__ labels, int* __restrict__ rec, int Hs, int Ws, int hw,
                                                           int K, int blocks_per_image, const unsigned char* __restrict__ band,
                                                           int* __restrict__ trec, int* __restrict__ arec, int* __restrict__ atab) {
  __shared__ int part[4][6];
  __shared__ unsigned int tb[4][TRIM_BUCKETS];         // TRIM: one bucket row per wave
  __shared__ int hist[AREA ? UNWARP_MAX_K : 1];        // AREA: predicted classes other than cl and K-1
  __shared__ int apart[4][AREA_REC];
  if (AREA) {
    for (int k = threadIdx.x; k < K; k += 256) hist[k] = 0;
  }
  if (TRIM) {
    if (threadIdx.x < 4 * TRIM_BUCKETS) tb[threadIdx.x / TRIM_BUCKETS][threadIdx.x % TRIM_BUCKETS] = 0u;
  }
  if (TRIM || AREA) __syncthreads();
  AreaWords aw = {{0u, 0u, 0u}, 0u};
  unsigned int* tbw = tb[threadIdx.x >> 6];
  const int b = blockIdx.x / blocks_per_image, chunk = blockIdx.x - b * blocks_per_image;
  const int per = Hs * Ws;
  const long base = (long)b * per;
  const int* ob = owner + base;
  const int* rx = rowx + base;
  const int* db = dec + (long)b * (hw + 1);
  const float* yb = yl + base;
  const long long cl = cls_label[b];
  const int bg = K - 1;
  AccCount n = {{0, 0, 0, 0, 0, 0}};
  const int p0 = chunk * UACC_CHUNK;
  if (VEC) {
#pragma unroll 1
    for (int j = 0; j < UACC_PIX / 4; ++j) {
      const int p = p0 + (j * 256 + (int)threadIdx.x) * 4;
      if (p >= per) break;                             // per % 4 == 0: the four pixels are in or out together
      const float4 y4 = *reinterpret_cast<const float4*>(yb + p);
      const int y = p / Ws, x = p - y * Ws;            // Ws % 4 == 0: one row
      int q[4];
      feeding_points4(ob, rx, y, x, Hs, Ws, hw, q);
      int a0 = db[q[0]], a1 = db[q[1]], a2 = db[q[2]], a3 = db[q[3]];
      if (AREA) {
        a0 = area_pixel(aw, hist, a0, y4.x, cl, bg); a1 = area_pixel(aw, hist, a1, y4.y, cl, bg);
        a2 = area_pixel(aw, hist, a2, y4.z, cl, bg); a3 = area_pixel(aw, hist, a3, y4.w, cl, bg);
      }
      count_pixel(n, a0, y4.x, cl, bg); count_pixel(n, a1, y4.y, cl, bg);
      count_pixel(n, a2, y4.z, cl, bg); count_pixel(n, a3, y4.w, cl, bg);
      if (TRIM) {
        const unsigned int b4 = *reinterpret_cast<const unsigned int*>(band + base + p);
        trim_pixel(tbw, b4 & 255u, a0, y4.x, cl, bg); trim_pixel(tbw, (b4 >> 8) & 255u, a1, y4.y, cl, bg);
        trim_pixel(tbw, (b4 >> 16) & 255u, a2, y4.z, cl, bg); trim_pixel(tbw, b4 >> 24, a3, y4.w, cl, bg);
      }
      if (labels != nullptr) {
        longlong2* lp = reinterpret_cast<longlong2*>(labels + base + p);
        lp[0] = make_longlong2(a0, a1); lp[1] = make_longlong2(a2, a3);
      }
    }
  } else {
#pragma unroll 1
    for (int j = 0; j < UACC_PIX; ++j) {
      const int p = p0 + j * 256 + (int)threadIdx.x;
      if (p >= per) break;
      const int y = p / Ws, x = p - y * Ws;
      int a = db[feeding_point(ob, rx, ob[p], y, x, Hs, Ws, hw)];
      if (AREA) a = area_pixel(aw, hist, a, yb[p], cl, bg);
      count_pixel(n, a, yb[p], cl, bg);
      if (TRIM) trim_pixel(tbw, band[base + p], a, yb[p], cl, bg);
      if (labels != nullptr) labels[base + p] = (long long)a;
    }
  }
  // in the wave by shuffles, across the four waves through LDS; integers: the same record whatever the order
#pragma unroll
  for (int q = 0; q < 6; ++q) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n.c[q] += __shfl_xor(n.c[q], o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int q = 0; q < 6; ++q) part[threadIdx.x >> 6][q] = n.c[q];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int s[6];
#pragma unroll
    for (int q = 0; q < 6; ++q) s[q] = (part[0][q] + part[1][q]) + (part[2][q] + part[3][q]);
    int4* r = reinterpret_cast<int4*>(rec + (long)blockIdx.x * UACC_REC);
    r[0] = make_int4(s[0], s[1], s[2], s[3]);
    r[1] = make_int4(s[4], s[5], 0, 0);
  }
  if (TRIM && threadIdx.x < TRIM_REC) {
    const int bi = threadIdx.x / 3, sh = 10 * (threadIdx.x % 3);
    int t = 0;
#pragma unroll
    for (int wv = 0; wv < 4; ++wv) t += (int)((tb[wv][bi] >> sh) & 1023u);
    trec[(long)blockIdx.x * TRIM_REC + threadIdx.x] = t;
  }
  if (AREA) {
#pragma unroll
    for (int q = 0; q < 3; ++q) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) aw.w[q] += __shfl_xor(aw.w[q], o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
      int* ap = apart[threadIdx.x >> 6];
#pragma unroll
      for (int f = 0; f < AREA_REC; ++f) ap[f] = (int)((aw.w[f / 3] >> (10 * (f % 3))) & 1023u);
    }
    // the barrier also ends the histogram's adds; no workgroup leaves before it (the trips above end by break, not return)
    const int cold = __syncthreads_or((int)aw.cold);
    if (threadIdx.x == 0) {
      int s[AREA_REC];
#pragma unroll
      for (int f = 0; f < AREA_REC; ++f) s[f] = (apart[0][f] + apart[1][f]) + (apart[2][f] + apart[3][f]);
      int4* r = reinterpret_cast<int4*>(arec + (long)blockIdx.x * AREA_REC);
      r[0] = make_int4(s[0], s[1], s[2], s[3]);
      r[1] = make_int4(s[4], s[5], s[6], s[7]);
    }
    if (cold) {
      for (int k = threadIdx.x; k < K; k += 256) {
        const int v = hist[k];
        if (v != 0) atomicAdd(atab + (long)b * K + k, v);
      }
    }
  }
}
// Class areas in the sampled space (eval.py:197, pred_deformed against y_sampled), and the ceiling bit of dec.  One workgroup per
// image.  At grid point p < h*w the prediction is pred[b,k,p] = cls[b,k] for k < K-1 and fmul(cls[b,K-1], m[b,p]) for K-1 -- one
// rounded multiply, as pred_assemble_fwd_kernel's -- and its class the first maximal k, NaN counting as maximal (torch.max).  The
// planes below K-1 are constant, so their first maximum kb is one per image and a point's class is kb or K-1; its label gs[p] is cl
// or K-1.  Only those classes can occur: four block-wide counts make every row of areas[b,2], and no histogram is needed.  ts[p] =
// (long)bilinear(y, grid[p]) is grid_sample_label_kernel's sequence (make_taps + sample_plane); it is or-ed into bit DEC_TS_BIT of
// dec[b,p] for the AREA count pass.  dec[b,h*w] keeps a clear bit: background.
__global__ __launch_bounds__(256) void class_area_sampled_kernel(const float* __restrict__ cls, const float* __restrict__ m,
                                                                 const float* __restrict__ grid, const float* __restrict__ yl,
                                                                 const long long* __restrict__ cls_label, int* __restrict__ dec,
                                                                 long long* __restrict__ areas, int K, int hw, int Hs, int Ws) {
  __shared__ float cs[UNWARP_MAX_K];
  __shared__ int kbest;
  __shared__ long long red[16];
  const int b = blockIdx.x;
  for (int k = threadIdx.x; k < K; k += 256) cs[k] = cls[(long)b * K + k];
  __syncthreads();
  if (threadIdx.x == 0) {
    float best = 0.f;
    int arg = 0;
    for (int k = 0; k < K - 1; ++k) {
      const float v = cs[k];
      if (k == 0 || v > best || (v != v && best == best)) { best = v; arg = k; }
    }
    kbest = arg;
  }
  __syncthreads();
  const int kb = kbest, bg = K - 1;
  const float best = cs[kb], c = cs[bg];
  const long long cl = cls_label[b];
  const float* mp = m + (long)b * hw;
  const float* gp = grid + 2 * (long)b * hw;
  const float* yb = yl + (long)b * Hs * Ws;
  int* db = dec + (long)b * (hw + 1);
  long long n[4] = {0, 0, 0, 0};                       // class K-1, ts, class == cl & ts, class == K-1 & !ts
  for (int p = threadIdx.x; p < hw; p += 256) {
    const Taps t = make_taps(gp[2 * p], gp[2 * p + 1], Hs, Ws);
    const int ts = (long long)sample_plane(yb, Ws, t) != 0;
    db[p] |= ts << DEC_TS_BIT;
    const float v = __fmul_rn(c, mp[p]);
    const int a = (v > best || (v != v && best == best)) ? bg : kb;
    n[0] += a == bg; n[1] += ts; n[2] += ((long long)a == cl) & ts; n[3] += (a == bg) & (ts ^ 1);
  }
  for (int q = 0; q < 4; ++q) n[q] = block_sum<long long>(n[q], red);
  long long* out = areas + ((long)b * 3 + 2) * K * 3;
  for (int k = threadIdx.x; k < K; k += 256) {
    const bool iscl = (long long)k == cl, isbg = k == bg;
    out[3 * k + 0] = (iscl ? n[2] : 0) + (isbg ? n[3] : 0);
    out[3 * k + 1] = (k == kb ? (long long)hw - n[0] : 0) + (isbg ? n[0] : 0);
    out[3 * k + 2] = (iscl ? n[1] : 0) + (isbg ? (long long)hw - n[1] : 0);
  }
}
// areas[b, 0] (prediction) and areas[b, 1] (ceiling) at full resolution = image b's hot records summed, the rows of the two hot
// classes made from them by equality (cl == K-1 merges into one row, cl outside 0 .. K-1 has none), plus atab's other predicted
// classes; one workgroup per image.  Record fields: AREA_REC.
__global__ __launch_bounds__(256) void unwarp_area_finalize_kernel(const int* __restrict__ arec, const int* __restrict__ atab,
                                                                   const long long* __restrict__ cls_label, long long* __restrict__ areas,
                                                                   int K, int blocks_per_image, long long per) {
  __shared__ long long red[16];
  const int b = blockIdx.x;
  const int4* r = reinterpret_cast<const int4*>(arec + (long)b * blocks_per_image * AREA_REC);
  long long c[AREA_REC] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int j = threadIdx.x; j < blocks_per_image; j += 256) {
    const int4 lo = r[2 * j], hi = r[2 * j + 1];
    c[0] += lo.x; c[1] += lo.y; c[2] += lo.z; c[3] += lo.w; c[4] += hi.x; c[5] += hi.y; c[6] += hi.z; c[7] += hi.w;
  }
  for (int q = 0; q < AREA_REC; ++q) c[q] = block_sum<long long>(c[q], red);
  const long long cl = cls_label[b];
  const int bg = K - 1;
  long long* o0 = areas + (long)b * 3 * K * 3;
  long long* o1 = o0 + (long)K * 3;
  for (int k = threadIdx.x; k < K; k += 256) {
    const bool iscl = (long long)k == cl, isbg = k == bg;
    const long long lab = (iscl ? c[0] : 0) + (isbg ? per - c[0] : 0);
    o0[3 * k + 0] = (iscl ? c[1] : 0) + (isbg ? c[2] : 0);
    o0[3 * k + 1] = (long long)atab[(long)b * K + k] + ((iscl && !isbg) ? c[3] : 0) + (isbg ? c[4] : 0);
    o0[3 * k + 2] = lab;
    // the ceiling predicts cl where ts, K-1 elsewhere: with cl == K-1 every pixel is predicted, labelled and right in that one row
    o1[3 * k + 0] = (iscl && isbg) ? per : (iscl ? c[6] : 0) + (isbg ? c[7] : 0);
    o1[3 * k + 1] = (iscl ? c[5] : 0) + (isbg ? per - c[5] : 0);
    o1[3 * k + 2] = lab;
  }
}
// trim[b, i, 0..3) = (total, cls_ok, bin_ok) of band i = the buckets 0 .. i of image b's records summed; one workgroup per image
__global__ __launch_bounds__(256) void unwarp_trim_finalize_kernel(const int* __restrict__ trec, long long* __restrict__ trim,
                                                                   int blocks_per_image, int D) {
  constexpr int G = 256 / TRIM_REC;                    // record rows in flight: thread (g, q) sums field q of rows g, g + G, ...
  __shared__ long long red[G][TRIM_REC];
  const int b = blockIdx.x, q = threadIdx.x % TRIM_REC, g = threadIdx.x / TRIM_REC;
  if (g < G) {
    long long s = 0;
    for (int j = g; j < blocks_per_image; j += G) s += trec[((long)b * blocks_per_image + j) * TRIM_REC + q];
    red[g][q] = s;
  }
  __syncthreads();
  if ((int)threadIdx.x < 3 * (D + 1)) {
    const int i = threadIdx.x / 3, f = threadIdx.x % 3;
    long long c = 0;
    for (int k = 0; k <= i; ++k)
      for (int r = 0; r < G; ++r) c += red[r][k * 3 + f];
    trim[((long)b * (D + 1) + i) * 3 + f] = c;
  }
}
// counts[b, 0..6) = the sum of image b's records; one workgroup per image
__global__ __launch_bounds__(256) void unwarp_count_finalize_kernel(const int* __restrict__ rec, long long* __restrict__ counts,
                                                                    int blocks_per_image) {
  __shared__ long long red[16];
  const int b = blockIdx.x;
  const int4* r = reinterpret_cast<const int4*>(rec + (long)b * blocks_per_image * UACC_REC);
  long long c[6] = {0, 0, 0, 0, 0, 0};
  for (int j = threadIdx.x; j < blocks_per_image; j += 256) {
    const int4 lo = r[2 * j], hi = r[2 * j + 1];
    c[0] += lo.x; c[1] += lo.y; c[2] += lo.z; c[3] += lo.w; c[4] += hi.x; c[5] += hi.y;
  }
  for (int q = 0; q < 6; ++q) {
    const long long s = block_sum<long long>(c[q], red);
    if (threadIdx.x == 0) counts[(long)b * 6 + q] = s;
  }
}
// acc[0..4) = acc, acc_bin_fg, acc_cls_fbg, acc_bin_fbg: seg_loss_finalize_kernel's arithmetic (head_loss.hip) on the integer counts
__global__ __launch_bounds__(256) void unwarp_accuracy_kernel(const long long* __restrict__ counts, float* __restrict__ acc, int B) {
  __shared__ double img[4][16];
  double a[4] = {0, 0, 0, 0};
  for (int b = threadIdx.x; b < B; b += blockDim.x) {
    const long long* c = counts + (long)b * 6;
    const float ufg = (float)c[2] + 1e-10f, ubg = (float)c[5] + 1e-10f;
    const float cls_fg = (float)c[0] / ufg, bin_fg = (float)c[1] / ufg, cls_bg = (float)c[3] / ubg, bin_bg = (float)c[4] / ubg;
    a[0] += cls_fg; a[1] += bin_fg; a[2] += cls_fg * 0.5f + cls_bg * 0.5f; a[3] += bin_fg * 0.5f + bin_bg * 0.5f;
  }
  for (int j = 0; j < 4; ++j) a[j] = block_sum<double>(a[j], img[j]);
  if (threadIdx.x < 4) {
    const int j = threadIdx.x;
    acc[j] = (float)((j == 0 ? a[0] : j == 1 ? a[1] : j == 2 ? a[2] : a[3]) / (double)B);
  }
}

// ---- trimap bands: which band of width 1, 2, 4 .. 2^D around the label's boundary a pixel lies in (eval.py:41-67) -------------------
// The reference dilates PIL's FIND_EDGES of the label 2^i times with scipy's cross element: an L1 distance threshold.  Here: seed =
// background pixel (t = (long)y == 0) with a foreground 8-neighbour (outside the image counts as background; with `frame` every
// background pixel of the outer ring is a seed, PIL copying the ring through unfiltered), d = L1 distance to the nearest seed, band =
// the smallest i with d <= 2^i, 255 if none.  The L1 distance separates: a row pass, then a column pass over its result.  Only
// d <= 2^D matters, so both passes keep bytes capped at 2^D + 1 and look no further than 2^D: a tile with that halo needs no carry.
// Inside a tile the 1-D pass is D + 1 doubling steps f[j] = min(f[j], f[j -+ s] + s), s = 1, 2 .. 2^D: a run of steps costs at least the
// offset it covers and the binary digits of an offset cost exactly it, so after them f[j] = min over |o| < 2^(D+1) of g[j+o] + |o|,
// exact; what a step reads from beyond the tile is missing, which only ever leaves an upper bound standing beside the exact one.
constexpr int TRI_MAX_D = 7;
constexpr int TRI_MAX_HALO = 1 << TRI_MAX_D;
constexpr int TRI_RG = 8;                              // row pass: rows per workgroup (ten rows of y read for eight written)
constexpr int TRI_SEG = 1024;                          // row pass: columns per workgroup
constexpr int TRI_MAX_HW = TRI_MAX_HALO / 64 + 1;      // row pass: 64-column words of halo on either side (64 * words > 2^D)
constexpr int TRI_NWORDS = TRI_SEG / 64 + 2 * TRI_MAX_HW;
constexpr int TRI_CW = 64;                             // column pass: columns per workgroup (sixteen 4-byte words a row)
constexpr int TRI_CH = 128;                            // column pass: rows per workgroup
constexpr int TRI_FAR = 1 << 20;
// row pass: inter[b, v, u] (row pitch P, a multiple of 4) = min(2^D + 1, distance along row v to the nearest seed).  A row is a string
// of bits, 64 columns a word: a wave's ballot makes a word of foreground bits from one coalesced read of y, the seed rule is shifts
// and ORs of three rows' words, and a pixel's distance is a count of leading / trailing zeros from its bit.
__global__ __launch_bounds__(256) void trimap_row_kernel(const float* __restrict__ y, unsigned char* __restrict__ inter, int Hs, int Ws, int P,
                                                         int D, int frame, int rgs, int segs) {
  __shared__ unsigned long long fgw[TRI_RG + 2][TRI_NWORDS];
  __shared__ unsigned long long sdw[TRI_RG][TRI_NWORDS];
  const int seg = blockIdx.x % segs, rg = (blockIdx.x / segs) % rgs, b = blockIdx.x / (segs * rgs);
  const int halo = 1 << D, cap = halo + 1, hw = halo / 64 + 1;
  const int segw = min(TRI_SEG, Ws - seg * TRI_SEG), nwords = (segw + 63) / 64 + 2 * hw;
  const int x0 = seg * TRI_SEG - 64 * hw, v0 = rg * TRI_RG;     // bit j of word k of a row is image column x0 + 64 k + j
  const int rows = min(TRI_RG, Hs - v0);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* yb = y + (long)b * Hs * Ws;
  for (int it = wave; it < (rows + 2) * nwords; it += 4) {
    const int r = it / nwords, k = it - r * nwords;
    const int v = v0 - 1 + r, u = x0 + 64 * k + lane;
    bool f = false;
    if (v >= 0 && v < Hs && u >= 0 && u < Ws) f = (long long)yb[(long)v * Ws + u] != 0;
    const unsigned long long bits = __ballot(f);
    if (lane == 0) fgw[r][k] = bits;
  }
  __syncthreads();
  for (int it = threadIdx.x; it < rows * nwords; it += 256) {
    const int r = it / nwords, k = it - r * nwords;
    const int v = v0 + r, ulo = x0 + 64 * k;
    const unsigned long long a = fgw[r][k] | fgw[r + 1][k] | fgw[r + 2][k];
    const unsigned long long al = k > 0 ? fgw[r][k - 1] | fgw[r + 1][k - 1] | fgw[r + 2][k - 1] : 0ull;
    const unsigned long long ar = k + 1 < nwords ? fgw[r][k + 1] | fgw[r + 1][k + 1] | fgw[r + 2][k + 1] : 0ull;
    // the region's two outermost columns miss a neighbour; they lie 64 * hw > 2^D columns from the segment and cannot matter
    unsigned long long take = a | a << 1 | al >> 63 | a >> 1 | ar << 63;
    if (frame) {
      if (v == 0 || v == Hs - 1) take = ~0ull;
      if (ulo <= 0 && 0 < ulo + 64) take |= 1ull << (0 - ulo);
      if (ulo <= Ws - 1 && Ws - 1 < ulo + 64) take |= 1ull << (Ws - 1 - ulo);
    }
    const int lo = max(0, -ulo), hi = min(64, Ws - ulo);          // the word's columns inside the image: bits lo .. hi - 1
    unsigned long long in = 0ull;
    if (hi > lo) in = (hi - lo == 64 ? ~0ull : (1ull << (hi - lo)) - 1ull) << lo;
    sdw[r][k] = ~fgw[r + 1][k] & take & in;
  }
  __syncthreads();
  // four columns a thread and a store; the pitch's padding takes whatever lies beside the row, and the column pass never shows it
  const int words = (segw + 3) >> 2;
  if ((int)threadIdx.x >= words) return;
  const int c0 = 64 * hw + 4 * (int)threadIdx.x, w = c0 >> 6;
  for (int r = 0; r < rows; ++r) {
    const unsigned long long* s = sdw[r];
    const unsigned long long cw = w < nwords ? s[w] : 0ull;
    int before = TRI_FAR, after = TRI_FAR;                       // from bit 0 / bit 63 of word w to the nearest seed in the words beside it
    for (int k = 1; k <= hw; ++k)
      if (w - k >= 0 && s[w - k] != 0ull) { before = 64 * (k - 1) + 1 + __builtin_clzll(s[w - k]); break; }
    for (int k = 1; k <= hw; ++k)
      if (w + k < nwords && s[w + k] != 0ull) { after = 64 * (k - 1) + 1 + __builtin_ctzll(s[w + k]); break; }
    unsigned int wd = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int bb = (c0 & 63) + q;
      const unsigned long long ml = cw & (~0ull >> (63 - bb)), mr = cw & (~0ull << bb);
      const int dl = ml != 0ull ? bb - (63 - __builtin_clzll(ml)) : bb + before;
      const int dr = mr != 0ull ? __builtin_ctzll(mr) - bb : 63 - bb + after;
      wd |= (unsigned int)min(min(dl, dr), cap) << (8 * q);
    }
    reinterpret_cast<unsigned int*>(inter + ((long)b * Hs + v0 + r) * P + seg * TRI_SEG)[threadIdx.x] = wd;
  }
}
// column pass: band[b, v, u] from min(2^D + 1, min over dv of inter[b, v + dv, u] + |dv|); a thread holds four neighbouring columns
__global__ __launch_bounds__(256) void trimap_col_kernel(const unsigned char* __restrict__ inter, unsigned char* __restrict__ band, int Hs, int Ws,
                                                         int P, int D, int vec, int rts, int cts) {
  extern __shared__ unsigned int tri_dist[];                   // [2][TRI_CH + 2 * 2^D][TRI_CW / 4]: sized by the launch, for occupancy at small D
  constexpr int WPR = TRI_CW / 4;
  const int ct = blockIdx.x % cts, rt = (blockIdx.x / cts) % rts, b = blockIdx.x / (cts * rts);
  const int halo = 1 << D, cap = halo + 1, nrmax = TRI_CH + 2 * halo;
  const int v0 = rt * TRI_CH, th = min(TRI_CH, Hs - v0), nr = th + 2 * halo;
  const int wl = threadIdx.x % WPR, rl = threadIdx.x / WPR;      // this thread's word of a row, and its first row
  const int u0 = ct * TRI_CW + 4 * wl;
  auto dist = [&](int buf, int r) -> unsigned int& { return tri_dist[(buf * nrmax + r) * WPR + wl]; };
  const bool live = u0 < P;
  const unsigned char* ib = inter + (long)b * Hs * P;
  bool seen = false;
#pragma unroll 4
  for (int r = rl; r < nr; r += 256 / WPR) {
    const int v = v0 - halo + r;
    unsigned int wd = (unsigned int)cap * 0x01010101u;           // outside the image: no seed
    if (live && v >= 0 && v < Hs) wd = *reinterpret_cast<const unsigned int*>(ib + (long)v * P + u0);
    dist(0, r) = wd;
    seen |= live && wd != (unsigned int)cap * 0x01010101u;
  }
  unsigned char* bb = band + (long)b * Hs * Ws;
  auto store = [&](int v, unsigned int o) {
    if (vec) {
      *reinterpret_cast<unsigned int*>(bb + (long)v * Ws + u0) = o;
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (u0 + q < Ws) bb[(long)v * Ws + u0 + q] = (unsigned char)(o >> (8 * q));
    }
  };
  if (!__syncthreads_or(seen)) {                                 // no seed within 2^D of any row this tile read: in no band
    if (live)
      for (int r = halo + rl; r < halo + th; r += 256 / WPR) store(v0 - halo + r, 0xFFFFFFFFu);
    return;
  }
  int cur = 0;
  for (int s = 1; s <= halo; s <<= 1) {
    for (int r = rl; r < nr; r += 256 / WPR) {
      const unsigned int a = dist(cur, r);
      const unsigned int up = r >= s ? dist(cur, r - s) : 0xFFFFFFFFu, dn = r + s < nr ? dist(cur, r + s) : 0xFFFFFFFFu;
      unsigned int wd = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int m = min(min((int)((a >> (8 * q)) & 255u), cap), min((int)((up >> (8 * q)) & 255u), (int)((dn >> (8 * q)) & 255u)) + s);
        wd |= (unsigned int)m << (8 * q);
      }
      dist(cur ^ 1, r) = wd;
    }
    __syncthreads();
    cur ^= 1;
  }
  if (!live) return;
  for (int r = halo + rl; r < halo + th; r += 256 / WPR) {
    const unsigned int wd = dist(cur, r);
    unsigned int o = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int d = (int)((wd >> (8 * q)) & 255u);
      const unsigned int i = d > halo ? 255u : d <= 1 ? 0u : (unsigned int)(32 - __clz(d - 1));
      o |= i << (8 * q);
    }
    store(v0 - halo + r, o);
  }
}

// ---- surface distance between two masks: the Hausdorff percentile (HD95) of evaluate(hausdorff=...) ----------------------------------
// The published definition utils.py:25-101 was copied from, in 2-D (the reference's own function flattens both masks before it erodes
// them and is called by nothing): the border of a mask is its foreground with a background 4-neighbour, everything
// outside the image being background; every border pixel of one mask takes the Euclidean distance to the nearest border pixel of the
// other, in both directions; the two sets are pooled; np.percentile(., q) interpolates between two order statistics.  Squared
// distances between pixels are integers, so everything up to the caller's two square roots is integer work, and exact:
//   fg       one byte per pixel, bit 0 = predicted foreground, bit 1 = label foreground (unwarp_fg_kernel, or the caller's)
//   column   per mask the border bit, and g = the vertical distance to the nearest border pixel of the pixel's column (two sweeps)
//   row      a border pixel at (y, x) of one mask: d^2 = min over x' of (x - x')^2 + g_other(y, x')^2, the row of g in LDS; the scan
//            walks outwards and stops once dx^2 alone reaches the best value so far, which no later column can beat; beyond the
//            first few columns the wave scans together for one pixel at a time
//   select   a two-level radix select over the pooled d^2 of an image: the row pass runs twice, first counting d^2 >> 15 into a
//            histogram, whose prefix sums give the bucket of either rank, then counting the low 15 bits of the values in those buckets.
//            No list of distances exists at any size; integer atomics only, the same bits in any order.
// HD_SENT is g in a column without a border pixel.  With Hs, Ws <= MASK_MAX_SIDE = 16384 a true d^2 is at most 2 * 16383^2 < 2^29,
// HD_SENT^2 = 2^30 lies above every one of them, and dx^2 + HD_SENT^2 <= 16383^2 + 2^30 < 2^31 stays an int.
constexpr int HD_SENT = 32768;
constexpr int HD_L1_SHIFT = 15;                        // level 1: d^2 >> 15, at most 2^14 buckets
constexpr int HD_L2_BINS = 1 << HD_L1_SHIFT;           // level 2: the low 15 bits
constexpr int HD_CACHE = 1024;                         // row pass: the first bins of a histogram are counted in LDS, then flushed
constexpr int HD_NEAR = 8;                             // row pass: columns on either side a lane scans alone before the wave joins in

// fg[b,v,u]: bit 0 = the class dec[feeding_point] is not K-1, bit 1 = the label mask's truncation is not 0.  dec may carry
// class_area_sampled_kernel's bit.  VEC: Ws % 4 == 0, y 16-byte aligned: four neighbours of one row, one word stored.
template <bool VEC>
__global__ __launch_bounds__(256) void unwarp_fg_kernel(const int* __restrict__ owner, const int* __restrict__ rowx, const int* __restrict__ dec,
                                                        const float* __restrict__ yl, unsigned char* __restrict__ fg, int Hs, int Ws, int hw,
                                                        int K, int blocks_per_image) {
  const int b = blockIdx.x / blocks_per_image, chunk = blockIdx.x - b * blocks_per_image;
  const int per = Hs * Ws;
  const long base = (long)b * per;
  const int* ob = owner + base;
  const int* rx = rowx + base;
  const int* db = dec + (long)b * (hw + 1);
  const float* yb = yl + base;
  const int bg = K - 1;
  const int p0 = chunk * UACC_CHUNK;
  if (VEC) {
    const int p = p0 + (int)threadIdx.x * 4;
    if (p >= per) return;
    const float4 y4 = *reinterpret_cast<const float4*>(yb + p);
    const int y = p / Ws, x = p - y * Ws;
    int q[4];
    feeding_points4(ob, rx, y, x, Hs, Ws, hw, q);
    const float ys[4] = {y4.x, y4.y, y4.z, y4.w};
    unsigned int wd = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned int pf = (db[q[k]] & DEC_CLASS_MASK) != bg, lf = (long long)ys[k] != 0;
      wd |= (pf | lf << 1) << (8 * k);
    }
    *reinterpret_cast<unsigned int*>(fg + base + p) = wd;
  } else {
#pragma unroll 1
    for (int j = 0; j < UACC_PIX; ++j) {
      const int p = p0 + j * 256 + (int)threadIdx.x;
      if (p >= per) break;
      const int y = p / Ws, x = p - y * Ws;
      const int a = db[feeding_point(ob, rx, ob[p], y, x, Hs, Ws, hw)] & DEC_CLASS_MASK;
      fg[base + p] = (unsigned char)((a != bg) | ((long long)yb[p] != 0) << 1);
    }
  }
}

// column pass: a thread per column (coalesced across x).  Downwards: the border bits of both masks from the byte and its four
// neighbours, g = rows since the last border pixel (HD_SENT before the first), both masks' g in one word (low half: bit 0's mask);
// upwards: the minimum with the rows until the next one.  cnt[b][2] += the border pixels of either mask.
__global__ __launch_bounds__(256) void hd_column_kernel(const unsigned char* __restrict__ fg, unsigned int* __restrict__ g, int* __restrict__ cnt,
                                                        int Hs, int Ws, int xblocks) {
  const int b = blockIdx.x / xblocks, x = (blockIdx.x - b * xblocks) * 256 + (int)threadIdx.x;
  int n0 = 0, n1 = 0;
  if (x < Ws) {
    const unsigned char* f = fg + (long)b * Hs * Ws + x;
    unsigned int* gb = g + (long)b * Hs * Ws + x;
    const bool hasl = x > 0, hasr = x + 1 < Ws;
    unsigned int up = 0u, c = f[0];
    int d0 = HD_SENT, d1 = HD_SENT;
    for (int y = 0; y < Hs; ++y) {
      const long o = (long)y * Ws;
      const unsigned int dn = y + 1 < Hs ? f[o + Ws] : 0u;
      const unsigned int l = hasl ? f[o - 1] : 0u, r = hasr ? f[o + 1] : 0u;
      const unsigned int bd = c & ~(up & dn & l & r) & 3u;
      d0 = (bd & 1u) ? 0 : (d0 == HD_SENT ? HD_SENT : d0 + 1);
      d1 = (bd & 2u) ? 0 : (d1 == HD_SENT ? HD_SENT : d1 + 1);
      n0 += (int)(bd & 1u); n1 += (int)(bd >> 1);
      gb[o] = (unsigned int)d0 | (unsigned int)d1 << 16;
      up = c; c = dn;
    }
    d0 = HD_SENT, d1 = HD_SENT;
    for (int y = Hs - 1; y >= 0; --y) {
      const long o = (long)y * Ws;
      const unsigned int v = gb[o];
      const int a0 = (int)(v & 0xFFFFu), a1 = (int)(v >> 16);
      d0 = a0 == 0 ? 0 : (d0 == HD_SENT ? HD_SENT : d0 + 1);
      d1 = a1 == 0 ? 0 : (d1 == HD_SENT ? HD_SENT : d1 + 1);
      const unsigned int wd = (unsigned int)min(a0, d0) | (unsigned int)min(a1, d1) << 16;
      if (wd != v) gb[o] = wd;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { n0 += __shfl_xor(n0, o, 64); n1 += __shfl_xor(n1, o, 64); }
  if ((threadIdx.x & 63) == 0) {
    if (n0) atomicAdd(cnt + 2 * b, n0);
    if (n1) atomicAdd(cnt + 2 * b + 1, n1);
  }
}

// row pass: one workgroup per image row, the row of g in LDS.  LEVEL 1: hist[b][d^2 >> 15] += 1 for every border pixel of either
// mask; LEVEL 2: hist[b][0 / 1][d^2 & 32767] += 1 for those whose d^2 >> 15 is the bucket of the lower / upper rank (sel[b][0], [2]).
// nb = bins of one histogram.  An image with an empty border has no distances: its rows return at once.
template <int LEVEL>
__global__ __launch_bounds__(256) void hd_row_kernel(const unsigned int* __restrict__ g, const int* __restrict__ cnt, const int* __restrict__ sel,
                                                     int* __restrict__ hist, int Hs, int Ws, int nb) {
  extern __shared__ unsigned int hd_row[];             // [Ws]
  __shared__ int cache[LEVEL][HD_CACHE];
  const int b = blockIdx.x / Hs;
  if (cnt[2 * b] == 0 || cnt[2 * b + 1] == 0) return;
  const unsigned int* gr = g + (long)blockIdx.x * Ws;
  int any = 0;
  for (int x = threadIdx.x; x < Ws; x += 256) {
    const unsigned int v = gr[x];
    hd_row[x] = v;
    any |= (v & 0xFFFFu) == 0u || (v >> 16) == 0u;
  }
  for (int i = threadIdx.x; i < LEVEL * HD_CACHE; i += 256) (&cache[0][0])[i] = 0;
  if (!__syncthreads_or(any)) return;                  // no border pixel in this row
  int b0 = 0, b1 = 0;
  if (LEVEL == 2) b0 = sel[4 * b], b1 = sel[4 * b + 2];
  int* h = hist + (long)b * LEVEL * nb;
  auto emit = [&](int best) {
    if (LEVEL == 1) {
      const int bin = best >> HD_L1_SHIFT;
      if (bin < HD_CACHE) atomicAdd(&cache[0][bin], 1);
      else if (bin < nb) atomicAdd(h + bin, 1);
    } else {
      const int hi = best >> HD_L1_SHIFT, bin = best & (HD_L2_BINS - 1);
      if (bin < nb) {
        if (hi == b0) { if (bin < HD_CACHE) atomicAdd(&cache[0][bin], 1); else atomicAdd(h + bin, 1); }
        if (hi == b1) { if (bin < HD_CACHE) atomicAdd(&cache[LEVEL - 1][bin], 1); else atomicAdd(h + nb + bin, 1); }
      }
    }
  };
  // A wave takes 64 neighbouring pixels at a time.  Every lane first scans the HD_NEAR columns on either side of its own pixel, which
  // settles nearly every pixel of a prediction near its label.  A pixel whose best value is still beyond HD_NEAR^2 is then scanned by the
  // whole wave, 256 columns on either side a trip (a lane takes four of them), until the nearest unseen column alone reaches the best
  // value: two border pixels in a row of 1024 cost sixteen trips, not a thousand steps of one lane.
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int c = wave; c * 64 < Ws; c += 4) {
    const int x = c * 64 + lane;
    const unsigned int v = x < Ws ? hd_row[x] : 0xFFFFFFFFu;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const bool isb = ((v >> (16 * k)) & 0xFFFFu) == 0u;   // a border pixel of mask k
      const int sh = 16 * (1 - k);                      // the other mask's half
      int best = 0x7FFFFFFF;
      if (isb) {
        const int g0 = (int)((v >> sh) & 0xFFFFu);
        best = g0 * g0;
        for (int dx = 1; dx <= HD_NEAR; ++dx) {
          const int dx2 = dx * dx;
          if (dx2 >= best) break;
          if (x - dx >= 0) { const int gg = (int)((hd_row[x - dx] >> sh) & 0xFFFFu); best = min(best, dx2 + gg * gg); }
          if (x + dx < Ws) { const int gg = (int)((hd_row[x + dx] >> sh) & 0xFFFFu); best = min(best, dx2 + gg * gg); }
        }
      }
      const bool more = isb && (HD_NEAR + 1) * (HD_NEAR + 1) < best && (x - (HD_NEAR + 1) >= 0 || x + (HD_NEAR + 1) < Ws);
      if (isb && !more) emit(best);
      unsigned long long pending = __ballot(more);
      while (pending != 0ull) {                         // uniform across the wave
        const int src = __builtin_ctzll(pending);
        pending &= pending - 1ull;
        const int xs = c * 64 + src;
        int bs = __shfl(best, src, 64);
        for (int base = HD_NEAR + 1; base < Ws; base += 256) {
          if (base * base >= bs || (xs - base < 0 && xs + base >= Ws)) break;
          int mine = bs;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int dx = base + 64 * j + lane, dx2 = dx * dx;
            if (dx2 < mine) {
              if (xs - dx >= 0) { const int gg = (int)((hd_row[xs - dx] >> sh) & 0xFFFFu); mine = min(mine, dx2 + gg * gg); }
              if (xs + dx < Ws) { const int gg = (int)((hd_row[xs + dx] >> sh) & 0xFFFFu); mine = min(mine, dx2 + gg * gg); }
            }
          }
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) mine = min(mine, __shfl_xor(mine, o, 64));
          bs = mine;
        }
        if (lane == src) emit(bs);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < LEVEL * HD_CACHE; i += 256) {
    const int which = i / HD_CACHE, bin = i - which * HD_CACHE;
    const int c = cache[which][bin];
    if (c != 0 && bin < nb) atomicAdd(h + (long)which * nb + bin, c);
  }
}

// the bin of h[0 .. nb) that holds the element of rank r (0-based, ascending; r < the histogram's total) -> out[0], and r's rank
// inside that bin -> out[1].  Block-wide, 256 threads; part = 256 ints of LDS.
__device__ __forceinline__ void hd_find_rank(const int* __restrict__ h, int nb, int r, int* out, int* part) {
  const int tid = threadIdx.x;
  const int seg = (nb + 255) / 256;
  const int x0 = min(tid * seg, nb), x1 = min(x0 + seg, nb);
  int s = 0;
  for (int i = x0; i < x1; ++i) s += h[i];
  __syncthreads();
  part[tid] = s;
  __syncthreads();
  if (tid == 0) {
    int c = 0;
    for (int t = 0; t < 256; ++t) { const int v = part[t]; part[t] = c; c += v; }
  }
  __syncthreads();
  int c = part[tid];
  if (r >= c && r < c + s) {
    for (int i = x0; i < x1; ++i) {
      const int v = h[i];
      if (r < c + v) { out[0] = i; out[1] = r - c; break; }
      c += v;
    }
  }
}
// n = n_pred + n_label pooled distances; np.percentile's two order statistics: ranks lo = q (n-1) div 100 and hi = lo + (a remainder).
// sel[b] = (bucket of lo, lo's rank in it, bucket of hi, hi's rank in it).  An empty border: hd[b] = (n_pred, n_label, -1, -1), final.
__global__ __launch_bounds__(256) void hd_select1_kernel(const int* __restrict__ cnt, const int* __restrict__ hist1, int* __restrict__ sel,
                                                         long long* __restrict__ hd, int nb1, int q) {
  __shared__ int part[256];
  const int b = blockIdx.x;
  const int n0 = cnt[2 * b], n1 = cnt[2 * b + 1];
  if (n0 == 0 || n1 == 0) {
    if (threadIdx.x == 0) { hd[4 * b] = n0; hd[4 * b + 1] = n1; hd[4 * b + 2] = -1; hd[4 * b + 3] = -1; }
    return;
  }
  const long long t = (long long)q * ((long long)n0 + n1 - 1);
  const int lo = (int)(t / 100), hi = lo + (t % 100 != 0);
  const int* h = hist1 + (long)b * nb1;
  hd_find_rank(h, nb1, lo, sel + 4 * b, part);
  hd_find_rank(h, nb1, hi, sel + 4 * b + 2, part);
}
// hd[b] = (n_pred, n_label, d2_lo, d2_hi): the bucket's high bits and the bin of the rank inside the bucket's histogram
__global__ __launch_bounds__(256) void hd_select2_kernel(const int* __restrict__ cnt, const int* __restrict__ hist2, const int* __restrict__ sel,
                                                         long long* __restrict__ hd, int nb2) {
  __shared__ int part[256];
  __shared__ int res[4];
  const int b = blockIdx.x;
  const int n0 = cnt[2 * b], n1 = cnt[2 * b + 1];
  if (n0 == 0 || n1 == 0) return;
  const int* h = hist2 + (long)b * 2 * nb2;
  hd_find_rank(h, nb2, sel[4 * b + 1], res, part);
  hd_find_rank(h + nb2, nb2, sel[4 * b + 3], res + 2, part);
  __syncthreads();
  if (threadIdx.x == 0) {
    hd[4 * b] = n0; hd[4 * b + 1] = n1;
    hd[4 * b + 2] = ((long long)sel[4 * b] << HD_L1_SHIFT) | res[0];
    hd[4 * b + 3] = ((long long)sel[4 * b + 2] << HD_L1_SHIFT) | res[2];
  }
}

// ---- the gazed instance as a record: bit mask, class, area, box and COCO run-length code (fs_unwarp_instances) ------------------------
// The label-free output without a class map.  The mask "class is not K-1" is gathered straight into bit words (mask_words.h: the layout
// and the word stores; the padding bits are stored clear), the statistics and the run-length code are made from the words by
// mask_rle.hip's passes, and the class is the head's own decision.
// head_fg_q_kernel's packed word of a grid point (the score section below): the foreground flag in the sign bit, q in the rest
constexpr int SCORE_FG_BIT = 31;
constexpr int SCORE_Q_MASK = 0x7fffffff;
struct GatherSum { unsigned int s; long b; };          // SCORE: the q of this thread's set pixels, and their image (-1: not live)
// The gather into bit words: bit (b, y, x) = the predicate of tab[b, feeding_point of the pixel], tab of hw + 1 words an image.
// Without SCORE tab is unwarp_decide_kernel's and the predicate "the class is not bg"; with it tab is head_fg_q_kernel's packed table,
// the predicate its sign bit, and the q of the set pixels is summed (a quad and a column lie in one row: one image a thread).
// VEC (Ws % 4 == 0, 16-byte aligned owner / rowx): four pixels a thread, eight lanes a word; else one lane a column.  No thread
// leaves before the store's shuffles / ballot.
template <bool VEC, bool SCORE>
__device__ __forceinline__ GatherSum gather_bits(const int* __restrict__ owner, const int* __restrict__ rowx, const int* __restrict__ tab,
                                                 unsigned int* __restrict__ bits, int Hs, int Ws, int P, int hw, int bg, long words) {
  constexpr int NPIX = VEC ? 4 : 1;
  const BitSlot sl = bit_slot<32 / NPIX>(Ws, P, words);
  GatherSum sum = {0u, -1};
  unsigned int set = 0u;                               // flag k: column x + k
  if (sl.live) {
    const int per = Hs * Ws;
    const long b = sl.row / Hs;
    const int y = (int)(sl.row - b * Hs);
    const int* ob = owner + b * per;
    const int* rx = rowx + b * per;
    const int* tb = tab + b * (hw + 1);
    int q[4];
    if (VEC) feeding_points4(ob, rx, y, sl.x, Hs, Ws, hw, q);
    else q[0] = feeding_point(ob, rx, ob[y * Ws + sl.x], y, sl.x, Hs, Ws, hw);
#pragma unroll
    for (int k = 0; k < NPIX; ++k) {
      const int wd = tb[q[k]];
      const bool f = SCORE ? wd < 0 : wd != bg;
      set |= (unsigned int)f << k;
      if (SCORE) sum.s += f ? (unsigned int)(wd & SCORE_Q_MASK) : 0u;
    }
    sum.b = b;
  }
  if (VEC) store_word_nibbles(bits, sl.g, words, set);
  else store_word_ballot(bits, sl.g, words, set != 0u);
  return sum;
}
template <bool VEC>
__global__ __launch_bounds__(256) void unwarp_bits_kernel(const int* __restrict__ owner, const int* __restrict__ rowx, const int* __restrict__ dec,
                                                          unsigned int* __restrict__ bits, int Hs, int Ws, int P, int hw, int K, long words) {
  gather_bits<VEC, false>(owner, rowx, dec, bits, Hs, Ws, P, hw, K - 1, words);
}
// cat[b] = the first maximal k < K-1 of cls[b,k], NaN maximal: unwarp_decide_kernel's comparison on the planes themselves
__global__ __launch_bounds__(256) void instance_cat_kernel(const float* __restrict__ cls, long long* __restrict__ cat, int B, int K) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const float* c = cls + (long)b * K;
  float best = 0.f;
  int arg = 0;
  for (int k = 0; k < K - 1; ++k) {
    const float v = c[k];
    if (k == 0 || v > best || (v != v && best == best)) { best = v; arg = k; }
  }
  cat[b] = arg;
}
// ---- the instance's confidence score (fs_head_fg_q, fs_unwarp_instances_scored; no counterpart in the reference: unpinned) -------------
// A pixel's foreground probability is the softmax mass of the classes below K-1 among the K values v[k] that unwarp_nearest(pred)
// holds there -- the values unwarp_decide_kernel takes the argmax of, so one number per feeding point: qt[b,p] = rint(2^24 * P),
// P = sum_{k<K-1} exp(v[k] - max v) / sum_{k<K} exp(v[k] - max v) in fp64 from the fp32 v; a NaN P (a NaN or +inf among the v, or all
// of them -inf) gives 0.  The v are unwarp_decide_kernel's float operations (same taps, same sample4); they are formed twice, for the
// maximum and for the sums, instead of being kept.  dec (nullable) = unwarp_decide_kernel's table: given, "class is not K-1" rides in
// bit SCORE_FG_BIT of the word, so that the scored gather reads one word per pixel as the unscored one reads dec.
constexpr double SCORE_ONE = 16777216.0;               // 2^24
__global__ __launch_bounds__(256) void head_fg_q_kernel(const float* __restrict__ cls, const float* __restrict__ m, const int* __restrict__ dec,
                                                        int* __restrict__ qt, int K, int h, int w, int blocks_per_image) {
  __shared__ float cs[UNWARP_MAX_K];
  const int b = blockIdx.x / blocks_per_image;
  const int hw = h * w;
  for (int k = threadIdx.x; k < K; k += 256) cs[k] = cls[(long)b * K + k];
  __syncthreads();
  const int p = (blockIdx.x - b * blocks_per_image) * 256 + threadIdx.x;
  if (p > hw) return;
  float gx = 0.f, gy = 0.f;
  if (p < hw) {
    const int yi = p / w, xi = p - yi * w;
    gx = __fsub_rn(__fmul_rn(__fdiv_rn((float)xi, (float)w), 2.f), 1.f);
    gy = __fsub_rn(__fmul_rn(__fdiv_rn((float)yi, (float)h), 2.f), 1.f);
  }
  const Taps t = make_taps(gx, gy, h, w);
  const bool inw = t.oky0 & t.okx0, ine = t.oky0 & t.okx1, isw = t.oky1 & t.okx0, ise = t.oky1 & t.okx1;
  auto sample4 = [&](float vnw, float vne, float vsw, float vse) {
    float acc = __fmul_rn(vnw, t.nw);
    acc = __fmaf_rn(vne, t.ne, acc);
    acc = __fmaf_rn(vsw, t.sw, acc);
    return __fmaf_rn(vse, t.se, acc);
  };
  auto plane = [&](float c) { return sample4(inw ? c : 0.f, ine ? c : 0.f, isw ? c : 0.f, ise ? c : 0.f); };
  const float c = cs[K - 1];
  const float* mp = m + (long)b * hw;
  const float vb = sample4(inw ? __fmul_rn(c, mp[t.y0 * w + t.x0]) : 0.f, ine ? __fmul_rn(c, mp[t.y0 * w + t.x0 + 1]) : 0.f,
                           isw ? __fmul_rn(c, mp[(t.y0 + 1) * w + t.x0]) : 0.f, ise ? __fmul_rn(c, mp[(t.y0 + 1) * w + t.x0 + 1]) : 0.f);
  float mx = vb;
  bool nan = vb != vb;
  for (int k = 0; k < K - 1; ++k) {
    const float v = plane(cs[k]);
    nan |= v != v;
    if (v > mx) mx = v;
  }
  double fg = 0.0;
  for (int k = 0; k < K - 1; ++k) fg += exp((double)plane(cs[k]) - (double)mx);
  const double P = fg / (fg + exp((double)vb - (double)mx));
  unsigned int word = (!nan && P == P) ? (unsigned int)(int)rint(P * SCORE_ONE) : 0u;
  const long i = (long)b * (hw + 1) + p;
  if (dec != nullptr) word |= (unsigned int)(dec[i] != K - 1) << SCORE_FG_BIT;
  qt[i] = (int)word;
}
// gather_bits from head_fg_q_kernel's packed table, and behind it the q of every set pixel summed per image.  A thread's sum is one
// image's.  A wave's words are consecutive -- WPW = 8 with VEC, 2 without -- so its images are
// those of its first to its last word: one, or two where it straddles an image's end, or more where an image has fewer words than a
// wave; bits past a row's end add nothing.  Per image the wave reduces by shuffles (a thread's sum is below 2^27, so 32 lanes fit 32
// bits and the last step is taken in 64; a wave without a set pixel of the image, the usual case of a small mask, skips them).  The
// sum of the wave's FIRST image goes to the wave's record by plain stores, written whatever its value -- rec[wave] as two 32-bit
// halves with VEC (256 pixels: up to 2^32), one int without (64 pixels: up to 2^30) -- and instance_conf_kernel sums an image's
// records in a fixed pass.  Only the sums of a wave's further images -- a straddling wave -- are added into qsum[b] (zeroed by the
// launcher) by 64-bit integer atomics, where non-zero; and every sum is where rec is null (the launcher: a scratch too misaligned
// for VEC at a width whose records were sized for it).  One atomic per wave or workgroup and
// image instead was measured: adds to 64 hot addresses serialise, 0.17 ms for a 7 150-pixel mask and 1.1 ms for a full one at B = 64
// (profiles/r21).  The waves are not joined: no barrier.  Integer sums: the same bits in any order.
template <bool VEC>
__global__ __launch_bounds__(256) void unwarp_bits_score_kernel(const int* __restrict__ owner, const int* __restrict__ rowx,
                                                                const int* __restrict__ qf, unsigned int* __restrict__ bits,
                                                                unsigned long long* __restrict__ qsum, int* __restrict__ rec, int Hs, int Ws,
                                                                int P, int hw, long words) {
  constexpr unsigned int WPW = VEC ? 8 : 2;            // words per wave: no more images than that
  const GatherSum mine = gather_bits<VEC, true>(owner, rowx, qf, bits, Hs, Ws, P, hw, 0, words);
  const unsigned int s = mine.s;
  const long tb = mine.b;                              // this thread's image
  // words < 2^27 (one lane a bit slot) and Hs * P < 2^31: 32-bit divisions
  const unsigned int wpi = (unsigned int)Hs * (unsigned int)P, nw = (unsigned int)words;
  const unsigned int wave = blockIdx.x * 4 + (threadIdx.x >> 6);
  const unsigned int g0 = wave * WPW;
  unsigned long long first = 0ull;
  if (g0 < nw) {
    const unsigned int g1 = (g0 + WPW < nw ? g0 + WPW : nw) - 1;
    const unsigned int b_lo = g0 / wpi, nimg = g1 / wpi - b_lo + 1;
    for (unsigned int i = 0; i < nimg; ++i) {
      unsigned int v = tb == (long)(b_lo + i) ? s : 0u;
      if (__ballot(v != 0u) == 0ull) continue;         // wave-uniform
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      const unsigned long long t = (unsigned long long)v + (unsigned long long)__shfl_xor(v, 32, 64);
      if (i == 0 && rec != nullptr) first = t;
      else if ((threadIdx.x & 63) == 0) atomicAdd(qsum + b_lo + i, t);
    }
  }
  if ((threadIdx.x & 63) == 0 && rec != nullptr) {
    if (VEC) { rec[2 * (long)wave] = (int)(unsigned int)first; rec[2 * (long)wave + 1] = (int)(unsigned int)(first >> 32); }
    else rec[wave] = (int)(unsigned int)first;
  }
}
// qsum[b] += the records of the waves whose first image is b -- wave v's first word is v * wpw, so they are the waves ceil(b * wpi / wpw)
// .. ceil((b+1) * wpi / wpw) - 1 -- summed by one workgroup per image in a fixed order; then
// conf[b] = (score, cls_prob, mask_prob): cls_prob = the fp64 softmax over cls[b, :K-1] at cat[b] (NaN where the row holds one),
// mask_prob = qsum / (area * 2^24) in fp64 (0 for an empty mask), score = their fp64 product; each rounded to fp32 once.  area =
// stats[b,0], rle_scan_kernel's.
__global__ __launch_bounds__(256) void instance_conf_kernel(const float* __restrict__ cls, const long long* __restrict__ cat,
                                                            const long long* __restrict__ stats, const int* __restrict__ rec,
                                                            long long* __restrict__ qsum, float* __restrict__ conf, int K, long wpi, int wpw,
                                                            long nwaves) {                   // wpw = 8: records of two ints, 2: of one
  __shared__ long long red[16];
  const int b = blockIdx.x;
  const long w0 = (b * wpi + wpw - 1) / wpw, w1e = ((b + 1) * wpi + wpw - 1) / wpw;
  const long w1 = w1e < nwaves ? w1e : nwaves;
  long long part = 0;
  if (rec != nullptr) {
    for (long v = w0 + threadIdx.x; v < w1; v += 256)
      part += wpw == 8 ? (long long)((unsigned long long)(unsigned int)rec[2 * v] | (unsigned long long)(unsigned int)rec[2 * v + 1] << 32)
                       : (long long)rec[v];
  }
  part = block_sum<long long>(part, red);
  if (threadIdx.x != 0) return;
  const long long q = qsum[b] + part;                  // the straddling waves' atomics are in already
  qsum[b] = q;
  const float* c = cls + (long)b * K;
  const int a = (int)cat[b];
  float mx = c[0];
  for (int k = 1; k < K - 1; ++k)
    if (c[k] > mx) mx = c[k];
  double sum = 0.0, ea = 0.0;
  for (int k = 0; k < K - 1; ++k) {
    const double e = exp((double)c[k] - (double)mx);
    sum += e;
    if (k == a) ea = e;
  }
  const double cp = ea / sum;
  const long long area = stats[(long)b * 6];
  const double mp = area > 0 ? (double)q / ((double)area * SCORE_ONE) : 0.0;
  conf[3 * b] = (float)(cp * mp); conf[3 * b + 1] = (float)cp; conf[3 * b + 2] = (float)mp;
}
// unwarp_bits_score_kernel's sums over the set bits of given words instead of the gathered ones (fs_unwarp_instances_component: the
// words are the component's, qf is head_fg_q_kernel's table).  One lane a word -- most words around one component are 0 and their
// lanes leave after one read; a lane with set bits walks them, and for each reads the table at the pixel's feeding_point.  A lane's sum is one image's and below 2^29.  The records are that kernel's with VEC: eight consecutive words (eight
// neighbouring lanes) make record g / 8, two ints, = the sum over those of the eight whose image is the first word's, by plain
// stores; a lane of a further image -- a group that straddles an image's end -- adds its sum into qsum (zeroed by the launcher) by a
// 64-bit integer atomic.  instance_conf_kernel sums the records with wpw = 8.  Integer sums: the same bits in any order.
__global__ __launch_bounds__(256) void component_qsum_kernel(const int* __restrict__ owner, const int* __restrict__ rowx, const int* __restrict__ qf,
                                                             const unsigned int* __restrict__ cbits, unsigned long long* __restrict__ qsum,
                                                             int* __restrict__ rec, int Hs, int Ws, int P, int hw, long words) {
  const int per = Hs * Ws;
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  const long wpi = (long)Hs * P;
  unsigned long long s = 0ull;
  long tb = -1;
  if (g < words) {
    const long row = g / P;
    const int c = (int)(g - row * P);
    unsigned int wd = cbits[g] & mask_tail(c, P, Ws);
    tb = row / Hs;
    if (wd != 0u) {
      const int y = (int)(row - tb * Hs);
      const int* ob = owner + tb * per;
      const int* rx = rowx + tb * per;
      const int* db = qf + tb * (hw + 1);
      while (wd != 0u) {
        const int x = 32 * c + __ffs((int)wd) - 1;
        wd &= wd - 1u;
        s += (unsigned int)(db[feeding_point(ob, rx, ob[y * Ws + x], y, x, Hs, Ws, hw)] & SCORE_Q_MASK);
      }
    }
  }
  const long g0 = g & ~7L;                              // the group's first word; the eight lanes are neighbours in one wave
  const long b0 = g0 < words ? g0 / wpi : -1;
  unsigned long long first = tb == b0 ? s : 0ull;
  first += __shfl_xor(first, 1, 64); first += __shfl_xor(first, 2, 64); first += __shfl_xor(first, 4, 64);
  if (tb != b0 && s != 0ull) atomicAdd(qsum + tb, s);
  if (g == g0 && g < words) { rec[2 * (g >> 3)] = (int)(unsigned int)first; rec[2 * (g >> 3) + 1] = (int)(unsigned int)(first >> 32); }
}

// ---- host: one plan, one job, one launcher -------------------------------------------------------------------------------------------
constexpr long INT_LIMIT = 2147483647L;                // pixel / point indices are ints (grid points and byte pitches too: not MASK_INT_LIMIT)
constexpr long TRI_WGS_MAX = 16777215L;                // the trimap passes' workgroups (256 threads each: fewer than 2^32 work-items)
inline bool row_fits_lds(int Ws) { return Ws <= 16384; }       // fill_row_nearest_kernel keeps one row of column indices in LDS
inline long align4(long v) { return (v + 3) & ~3L; }           // ints: the next 16-byte boundary

// fs_trimap_bands' sizes: the row pass's byte map has its rows pitched to four bytes
struct TrimapPlan {
  long P, rgs, segs, rts, cts;                         // pitch; row groups and segments of the row pass; row and column tiles of the column pass
  long ints;                                           // scratch of the row pass
  bool ok;                                             // launchable
};
TrimapPlan trimap_plan(int B, int Hs, int Ws) {
  TrimapPlan t = {};
  if (!(B > 0 && Hs > 0 && Ws > 0)) return t;
  t.P = align4(Ws);
  t.rgs = cdiv(Hs, TRI_RG), t.segs = cdiv(Ws, TRI_SEG), t.rts = cdiv(Hs, TRI_CH), t.cts = cdiv(t.P, TRI_CW);
  t.ints = (long)B * Hs * t.P / 4;
  t.ok = t.P < INT_LIMIT && (long)B * t.rgs * t.segs <= TRI_WGS_MAX && (long)B * t.rts * t.cts <= TRI_WGS_MAX;
  return t;
}

// fs_surface_hd's sizes.  Scratch, in ints: g [n] (both masks' column distances, two 16-bit halves a pixel), then the region zeroed
// before every call: cnt [B][2], sel [B][4], the level-1 histograms [B][nb1], the level-2 histograms [B][2][nb2].  The histograms are
// no longer than the image's largest d^2 = (Hs-1)^2 + (Ws-1)^2 needs.
struct SurfacePlan {
  long n, nb1, nb2;
  long g, cnt, sel, h1, h2, total;
  bool ok;                                             // launchable
};
SurfacePlan surface_plan(int B, int Hs, int Ws) {
  SurfacePlan s = {};
  if (!(B > 0 && Hs > 0 && Ws > 0)) return s;
  s.n = (long)B * Hs * Ws;
  const long maxd2 = (long)(Hs - 1) * (Hs - 1) + (long)(Ws - 1) * (Ws - 1);
  s.nb1 = (maxd2 >> HD_L1_SHIFT) + 1, s.nb2 = maxd2 + 1 < HD_L2_BINS ? maxd2 + 1 : HD_L2_BINS;
  s.g = 0, s.cnt = align4(s.n), s.sel = s.cnt + 2L * B, s.h1 = s.sel + 4L * B, s.h2 = s.h1 + (long)B * s.nb1;
  s.total = s.h2 + 2L * B * s.nb2;
  s.ok = Hs <= MASK_MAX_SIDE && Ws <= MASK_MAX_SIDE && (long)B * Hs * 256 <= THREADS_MAX && (long)B * cdiv(Ws, 256) * 256 <= THREADS_MAX;
  return s;
}

// What a call computes on top of the class-map gather.  UW_COUNT: the gather counts (fs_unwarp_accuracy); UW_TRIM / UW_AREA: it also
// buckets by trimap band / sums class areas; UW_HD: a foreground byte map and the surface distances behind the count pass.  Each
// feature appends its regions to the scratch of the one before; UW_AREA's layout keeps UW_TRIM's regions whether or not the call has a
// trimap, and UW_HD's come after whatever the other features of the call take.  UW_BITS (fs_unwarp_instances): the gather stores bit
// words instead of classes, and the run-length passes follow; its regions come last of all, and it goes with no counting feature.
// UW_SCORE (fs_unwarp_instances_scored): UW_BITS with the gather also summing the feeding points' foreground probabilities; its one
// regions, the packed table and the gather's per-wave records, come behind UW_BITS', whose layout stays what it is without it.
// UW_COMP (fs_unwarp_instances_component): UW_BITS with the connected component under the gaze taken from the gathered words before
// the run-length passes; with UW_SCORE the q sum is taken over the component's bits by a pass of its own (component_qsum_kernel) and the
// gather is the unscored one.  Its regions come behind everything else.
enum : unsigned { UW_LABELS = 0, UW_COUNT = 1, UW_TRIM = 2, UW_AREA = 4, UW_HD = 8, UW_BITS = 16, UW_SCORE = 32, UW_COMP = 64 };

struct UnwarpPlan {
  int B, K, h, w, Hs, Ws;
  unsigned features;
  long per, n;                                         // pixels per image, of the batch
  long bpi, cpi;                                       // workgroups per image: decide pass, count pass (= records)
  // scratch, in ints from its start (16-byte aligned where a region is stored or read 16 bytes at a time)
  long owner, rowx, dec;                               // [n], [n], [B*(h*w+1)]
  long rec;                                            // UW_COUNT: [B*cpi][UACC_REC]
  long trec, band, inter;                              // UW_TRIM: [B*cpi][TRIM_REC], n band bytes, TrimapPlan::ints
  long arec, atab;                                     // UW_AREA: [B*cpi][AREA_REC], [B][K] sums of the other predicted classes' pixels
  long fg, hds;                                        // UW_HD: n foreground bytes, SurfacePlan::total
  long bitw, rles;                                     // UW_BITS: RlePlan::words bit words (used when the caller keeps none), RlePlan::total
  long raww, cmps, crec;                               // UW_COMP: the gathered bit words, ComponentPlan::scratch, two ints per eight words: component_qsum_kernel's records
  ComponentPlan cmp;
  long qtab, srec;                                     // UW_SCORE: [B*(h*w+1)] head_fg_q_kernel's packed words; two ints per wave of the gather
  long total;
  TrimapPlan tri;
  SurfacePlan sp;
  RlePlan rle;
  bool ok;                                             // launchable: sizes and limits (pointers are the job's)
};
UnwarpPlan unwarp_plan(int B, int K, int h, int w, int Hs, int Ws, unsigned features) {
  UnwarpPlan p = {};
  p.B = B, p.K = K, p.h = h, p.w = w, p.Hs = Hs, p.Ws = Ws, p.features = features;
  if (!(B > 0 && h > 0 && w > 0 && Hs > 0 && Ws > 0 && (K > 0 || !(features & UW_AREA)))) return p;
  p.per = (long)Hs * Ws, p.n = (long)B * p.per;
  p.bpi = ((long)h * w + 1 + 255) / 256;
  p.cpi = (p.per + UACC_CHUNK - 1) / UACC_CHUNK;
  p.tri = trimap_plan(B, Hs, Ws);
  p.owner = 0, p.rowx = p.n, p.dec = 2 * p.n;
  p.total = p.dec + (long)B * ((long)h * w + 1);
  if (features & (UW_COUNT | UW_TRIM | UW_AREA)) p.rec = align4(p.total), p.total = p.rec + (long)B * p.cpi * UACC_REC;
  if (features & (UW_TRIM | UW_AREA)) {
    p.trec = align4(p.total), p.band = p.trec + (long)B * p.cpi * TRIM_REC, p.inter = p.band + align4((p.n + 3) / 4);
    p.total = p.inter + p.tri.ints;
  }
  if (features & UW_AREA) p.arec = align4(p.total), p.atab = p.arec + (long)B * p.cpi * AREA_REC, p.total = p.atab + (long)B * K;
  if (features & UW_HD) {
    p.sp = surface_plan(B, Hs, Ws);
    p.fg = align4(p.total), p.hds = p.fg + align4((p.n + 3) / 4), p.total = p.hds + p.sp.total;
  }
  if (features & UW_BITS) {
    p.rle = rle_plan(B, Hs, Ws);
    p.bitw = align4(p.total), p.rles = p.bitw + align4(p.rle.words), p.total = p.rles + p.rle.total;
  }
  // the gather's waves: four to a workgroup of 32 words and two ints each where Ws % 4 == 0, else four to one of 8 words and one int
  if (features & UW_SCORE)
    p.qtab = align4(p.total), p.srec = align4(p.qtab + (long)B * ((long)h * w + 1)),
    p.total = p.srec + (Ws % 4 == 0 ? 8 * ((p.rle.words + 31) / 32) : 4 * ((p.rle.words + 7) / 8));
  if (features & UW_COMP) {
    p.cmp = component_plan(B, Hs, Ws);
    p.raww = align4(p.total), p.cmps = p.raww + align4(p.rle.words), p.crec = p.cmps + align4(p.cmp.scratch);
    p.total = p.crec + 2 * ((p.rle.words + 7) / 8);
  }
  // a workgroup's last trip of the count pass may start up to a chunk past the end
  const long per_max = INT_LIMIT - (features & UW_COUNT ? UACC_CHUNK : 0);
  p.ok = K >= 2 && K <= UNWARP_MAX_K && row_fits_lds(Ws) && (long)h * w < INT_LIMIT && p.per < per_max && p.n <= THREADS_MAX &&
         (long)B * Hs * 256 <= THREADS_MAX && (long)B * p.bpi * 256 <= THREADS_MAX &&
         (!(features & UW_COUNT) || (long)B * p.cpi * 256 <= THREADS_MAX) && (!(features & UW_TRIM) || p.tri.ok) &&
         (!(features & UW_HD) || ((features & UW_COUNT) && p.sp.ok)) &&
         (!(features & UW_BITS) || ((features & ~(UW_SCORE | UW_COMP)) == UW_BITS && p.rle.bits_ok && p.rle.ok)) &&
         (!(features & UW_SCORE) || (features & UW_BITS)) && (!(features & UW_COMP) || ((features & UW_BITS) && p.cmp.ok));
  return p;
}

// The caller's pointers, in the order the entry points brace them: cls, m, grid and scratch always; then one group per feature.
struct UnwarpJob {
  const float *cls, *m, *grid;
  int* scratch;
  struct { long long* map; unsigned char* hole; } labels;                                       // map: required without UW_COUNT, optional with it
  struct { const float* y; const long long* cls_label; long long* counts; float* acc; } count;  // UW_COUNT
  struct { long long* out; int D, frame; } trim;                                                // UW_TRIM
  struct { long long* out; } areas;                                                             // UW_AREA
  struct { long long* out; int q; } hd;                                                         // UW_HD
  struct { long long *cat, *stats; int* counts; unsigned int* bits; int cap; float* conf; long long* qsum; } inst;   // UW_BITS; bits optional; conf, qsum: UW_SCORE
  struct { const float* focus; long long* out; int conn; long snap2; } comp;                    // UW_COMP
};

bool trimap_args_ok(int D, int frame) { return D >= 0 && D <= TRI_MAX_D && (frame == 0 || frame == 1); }

int trimap_launch(const TrimapPlan& t, const float* y, unsigned char* band, unsigned char* inter, int B, int Hs, int Ws, int D, int frame,
                  hipStream_t stream) {
  hipLaunchKernelGGL(trimap_row_kernel, dim3((unsigned)(B * t.rgs * t.segs)), dim3(256), 0, stream, y, inter, Hs, Ws, (int)t.P, D, frame,
                     (int)t.rgs, (int)t.segs);
  FS_LAUNCH_CHECK();
  const int vec = Ws % 4 == 0 && ((uintptr_t)band & 3) == 0;
  hipLaunchKernelGGL(trimap_col_kernel, dim3((unsigned)(B * t.rts * t.cts)), dim3(256), 2 * (TRI_CH + (2 << D)) * TRI_CW, stream, inter, band,
                     Hs, Ws, (int)t.P, D, vec, (int)t.rts, (int)t.cts);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

bool hd_args_ok(int q) { return q >= 1 && q <= 100; }

// zeroed counters and histograms, the column pass, then twice the row pass with a selection behind it
int surface_launch(const SurfacePlan& sp, const unsigned char* fg, long long* hd, int* s, int B, int Hs, int Ws, int q, hipStream_t stream) {
  const hipError_t e = hipMemsetAsync(s + sp.cnt, 0, sizeof(int) * (size_t)(sp.total - sp.cnt), stream);
  if (e != hipSuccess) return (int)e;
  unsigned int* g = reinterpret_cast<unsigned int*>(s + sp.g);
  const int xblocks = cdiv(Ws, 256);
  hipLaunchKernelGGL(hd_column_kernel, dim3((unsigned)(B * xblocks)), dim3(256), 0, stream, fg, g, s + sp.cnt, Hs, Ws, xblocks);
  FS_LAUNCH_CHECK();
  const int lds = Ws * (int)sizeof(unsigned int);
  if (lds > 48 * 1024) {                               // with the static histograms beside it the row is beyond the default
    static unsigned long long done1 = 0ull, done2 = 0ull;
    FS_TRY(fs_lds_opt_in(reinterpret_cast<const void*>(&hd_row_kernel<1>), lds, done1));
    FS_TRY(fs_lds_opt_in(reinterpret_cast<const void*>(&hd_row_kernel<2>), lds, done2));
  }
  hipLaunchKernelGGL(hd_row_kernel<1>, dim3((unsigned)((long)B * Hs)), dim3(256), (size_t)lds, stream, g, s + sp.cnt, s + sp.sel, s + sp.h1, Hs, Ws,
                     (int)sp.nb1);
  FS_LAUNCH_CHECK();
  hipLaunchKernelGGL(hd_select1_kernel, dim3((unsigned)B), dim3(256), 0, stream, s + sp.cnt, s + sp.h1, s + sp.sel, hd, (int)sp.nb1, q);
  FS_LAUNCH_CHECK();
  hipLaunchKernelGGL(hd_row_kernel<2>, dim3((unsigned)((long)B * Hs)), dim3(256), (size_t)lds, stream, g, s + sp.cnt, s + sp.sel, s + sp.h2, Hs, Ws,
                     (int)sp.nb2);
  FS_LAUNCH_CHECK();
  hipLaunchKernelGGL(hd_select2_kernel, dim3((unsigned)B), dim3(256), 0, stream, s + sp.cnt, s + sp.h2, s + sp.sel, hd, (int)sp.nb2);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

// owner = -1, then every grid point's claim
int claim_owners(const float* grid, int* owner, int B, int h, int w, int Hs, int Ws, hipStream_t stream) {
  const hipError_t e = hipMemsetAsync(owner, 0xFF, sizeof(int) * (size_t)B * Hs * Ws, stream);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(inverse_owner_kernel, dim3(cdiv((long)B * h * w, 256)), dim3(256), 0, stream, grid, owner, B, h * w, Hs, Ws);
  FS_LAUNCH_CHECK();
  return FS_OK;
}
int row_nearest_launch(const int* owner, int* rowx, int B, int Hs, int Ws, hipStream_t stream) {
  hipLaunchKernelGGL(fill_row_nearest_kernel, dim3((unsigned)((long)B * Hs)), dim3(256), (size_t)Ws * sizeof(int), stream, owner, rowx, Ws);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

// What every un-warp begins with: the decision per grid point (with UW_AREA class_area_sampled_kernel then tags dec, writes areas[:,2],
// and atab is zeroed for the count pass), the owner map, the nearest claimed column per row.
int unwarp_prelude(const UnwarpPlan& p, const UnwarpJob& j, hipStream_t stream) {
  int* s = j.scratch;
  hipLaunchKernelGGL(unwarp_decide_kernel, dim3((unsigned)(p.B * p.bpi)), dim3(256), 0, stream, j.cls, j.m, s + p.dec, p.K, p.h, p.w, (int)p.bpi);
  FS_LAUNCH_CHECK();
  if (p.features & UW_AREA) {
    hipLaunchKernelGGL(class_area_sampled_kernel, dim3((unsigned)p.B), dim3(256), 0, stream, j.cls, j.m, j.grid, j.count.y, j.count.cls_label,
                       s + p.dec, j.areas.out, p.K, p.h * p.w, p.Hs, p.Ws);
    FS_LAUNCH_CHECK();
    const hipError_t e = hipMemsetAsync(s + p.atab, 0, sizeof(int) * (size_t)p.B * p.K, stream);
    if (e != hipSuccess) return (int)e;
  }
  FS_TRY(claim_owners(j.grid, s + p.owner, p.B, p.h, p.w, p.Hs, p.Ws, stream));
  return row_nearest_launch(s + p.owner, s + p.rowx, p.B, p.Hs, p.Ws, stream);
}

// unwarp_count_kernel<VEC, TRIM, AREA> by index VEC + 2 * TRIM + 4 * AREA
using CountKernel = decltype(&unwarp_count_kernel<false, false, false>);
const CountKernel COUNT_KERNELS[8] = {
    unwarp_count_kernel<false, false, false>, unwarp_count_kernel<true, false, false>, unwarp_count_kernel<false, true, false>,
    unwarp_count_kernel<true, true, false>,   unwarp_count_kernel<false, false, true>, unwarp_count_kernel<true, false, true>,
    unwarp_count_kernel<false, true, true>,   unwarp_count_kernel<true, true, true>};

// The launches of the eight entry points: [trimap bands,] prelude, then either the class map, or with UW_BITS the instance sequence
// below, or the count pass and its finalizers (the trimap's and the areas' after the accuracies'), then with UW_HD the foreground
// bytes and the surface distances.
int unwarp_run(const UnwarpPlan& p, const UnwarpJob& j, hipStream_t stream) {
  const bool count = p.features & UW_COUNT, trim = p.features & UW_TRIM, area = p.features & UW_AREA, hdq = p.features & UW_HD;
  const bool inst = p.features & UW_BITS, score = p.features & UW_SCORE, comp = p.features & UW_COMP;
  FS_REQUIRE(p.ok && j.cls && j.m && j.grid && j.scratch && (count || inst || j.labels.map));
  FS_REQUIRE(!inst || (j.inst.cat && j.inst.stats && j.inst.counts && j.inst.cap >= 1));
  FS_REQUIRE(!score || (j.inst.conf && j.inst.qsum));
  FS_REQUIRE(!comp || (j.comp.focus && j.comp.out && (j.comp.conn == 4 || j.comp.conn == 8) && j.comp.snap2 >= 0));
  // the records are stored and read 16 bytes at a time
  FS_REQUIRE(!count || (j.count.y && j.count.cls_label && j.count.counts && j.count.acc && ((uintptr_t)j.scratch & 15) == 0));
  FS_REQUIRE((!trim || (j.trim.out && trimap_args_ok(j.trim.D, j.trim.frame))) && (!area || j.areas.out));
  FS_REQUIRE(!hdq || (j.hd.out && hd_args_ok(j.hd.q)));
  int* s = j.scratch;
  unsigned char* band = trim ? reinterpret_cast<unsigned char*>(s + p.band) : nullptr;
  if (trim) FS_TRY(trimap_launch(p.tri, j.count.y, band, reinterpret_cast<unsigned char*>(s + p.inter), p.B, p.Hs, p.Ws, j.trim.D, j.trim.frame, stream));
  FS_TRY(unwarp_prelude(p, j, stream));
  if (inst) {
    // The record -- words, run-length code, q sum -- is made from `bits`, the caller's words or scratch.  Without a component the gather
    // writes them, and a scored gather sums q as it goes.  With one the gather is the unscored one and its words stay in scratch; the
    // component's become `bits`, and the q sum is a pass of its own over them (component_qsum_kernel).
    unsigned int* bits = j.inst.bits ? j.inst.bits : reinterpret_cast<unsigned int*>(s + p.bitw);
    unsigned int* gathered = comp ? reinterpret_cast<unsigned int*>(s + p.raww) : bits;
    unsigned long long* qsum = reinterpret_cast<unsigned long long*>(j.inst.qsum);
    const bool fused = score && !comp;
    // four pixels a thread need whole 16-byte rows of owner and rowx
    const bool vec4 = p.Ws % 4 == 0 && ((uintptr_t)s & 15) == 0;
    const dim3 ggrid(cdiv(p.rle.words, vec4 ? 32 : 8));
    const int hw = p.h * p.w, P = (int)p.rle.P;
    // the route's q records for instance_conf_kernel: the component pass's, two ints per eight words; or the scored gather's, one per
    // wave of wpw words -- null where they were sized for the gather the width allows and the scratch's alignment forbids it
    int* qrec = comp ? s + p.crec : (p.Ws % 4 == 0) == vec4 ? s + p.srec : nullptr;
    const int wpw = comp || vec4 ? 8 : 2;
    const long nwaves = comp ? (long)cdiv(p.rle.words, 8) : 4L * cdiv(p.rle.words, 4 * wpw);
    if (score) {
      hipLaunchKernelGGL(head_fg_q_kernel, dim3((unsigned)(p.B * p.bpi)), dim3(256), 0, stream, j.cls, j.m, s + p.dec, s + p.qtab, p.K, p.h, p.w,
                         (int)p.bpi);
      FS_LAUNCH_CHECK();
    }
    if (fused) {
      const hipError_t e = hipMemsetAsync(qsum, 0, sizeof(long long) * (size_t)p.B, stream);
      if (e != hipSuccess) return (int)e;
      hipLaunchKernelGGL(vec4 ? unwarp_bits_score_kernel<true> : unwarp_bits_score_kernel<false>, ggrid, dim3(256), 0, stream, s + p.owner,
                         s + p.rowx, s + p.qtab, gathered, qsum, qrec, p.Hs, p.Ws, P, hw, p.rle.words);
    } else {
      hipLaunchKernelGGL(vec4 ? unwarp_bits_kernel<true> : unwarp_bits_kernel<false>, ggrid, dim3(256), 0, stream, s + p.owner, s + p.rowx,
                         s + p.dec, gathered, p.Hs, p.Ws, P, hw, p.K, p.rle.words);
    }
    FS_LAUNCH_CHECK();
    hipLaunchKernelGGL(instance_cat_kernel, dim3(cdiv(p.B, 256)), dim3(256), 0, stream, j.cls, j.inst.cat, p.B, p.K);
    FS_LAUNCH_CHECK();
    if (comp) FS_TRY(component_launch(p.cmp, gathered, j.comp.focus, bits, j.comp.out, s + p.cmps, p.B, p.Hs, p.Ws, j.comp.conn, j.comp.snap2, stream));
    FS_TRY(rle_launch(p.rle, bits, j.inst.stats, j.inst.counts, s + p.rles, p.B, p.Hs, p.Ws, j.inst.cap, stream));
    if (score && comp) {
      const hipError_t e = hipMemsetAsync(qsum, 0, sizeof(long long) * (size_t)p.B, stream);
      if (e != hipSuccess) return (int)e;
      hipLaunchKernelGGL(component_qsum_kernel, dim3(cdiv(p.rle.words, 256)), dim3(256), 0, stream, s + p.owner, s + p.rowx, s + p.qtab, bits, qsum,
                         qrec, p.Hs, p.Ws, P, hw, p.rle.words);
      FS_LAUNCH_CHECK();
    }
    if (score) {
      hipLaunchKernelGGL(instance_conf_kernel, dim3((unsigned)p.B), dim3(256), 0, stream, j.cls, j.inst.cat, j.inst.stats, qrec, j.inst.qsum,
                         j.inst.conf, p.K, (long)p.Hs * P, wpw, nwaves);
      FS_LAUNCH_CHECK();
    }
    return FS_OK;
  }
  if (!count) {
    hipLaunchKernelGGL(unwarp_label_kernel, dim3(cdiv(p.n, 256)), dim3(256), 0, stream, s + p.owner, s + p.rowx, s + p.dec, j.labels.map,
                       j.labels.hole, p.n, p.Hs, p.Ws, p.h * p.w);
    FS_LAUNCH_CHECK();
    return FS_OK;
  }
  int *rec = s + p.rec, *trec = trim ? s + p.trec : nullptr;
  int *arec = area ? s + p.arec : nullptr, *atab = area ? s + p.atab : nullptr;
  // four pixels a thread needs whole 16-byte rows of y and labels, and whole words of band
  const bool vec = p.Ws % 4 == 0 && ((uintptr_t)j.count.y & 15) == 0 && ((uintptr_t)j.labels.map & 15) == 0 && ((uintptr_t)band & 3) == 0;
  hipLaunchKernelGGL(COUNT_KERNELS[vec + 2 * trim + 4 * area], dim3((unsigned)(p.B * p.cpi)), dim3(256), 0, stream, s + p.owner, s + p.rowx,
                     s + p.dec, j.count.y, j.count.cls_label, j.labels.map, rec, p.Hs, p.Ws, p.h * p.w, p.K, (int)p.cpi, band, trec, arec, atab);
  FS_LAUNCH_CHECK();
  hipLaunchKernelGGL(unwarp_count_finalize_kernel, dim3((unsigned)p.B), dim3(256), 0, stream, rec, j.count.counts, (int)p.cpi);
  FS_LAUNCH_CHECK();
  hipLaunchKernelGGL(unwarp_accuracy_kernel, dim3(1), dim3(256), 0, stream, j.count.counts, j.count.acc, p.B);
  FS_LAUNCH_CHECK();
  if (trim) {
    hipLaunchKernelGGL(unwarp_trim_finalize_kernel, dim3((unsigned)p.B), dim3(256), 0, stream, trec, j.trim.out, (int)p.cpi, j.trim.D);
    FS_LAUNCH_CHECK();
  }
  if (area) {
    hipLaunchKernelGGL(unwarp_area_finalize_kernel, dim3((unsigned)p.B), dim3(256), 0, stream, arec, atab, j.count.cls_label, j.areas.out, p.K,
                       (int)p.cpi, (long long)p.per);
    FS_LAUNCH_CHECK();
  }
  if (hdq) {
    unsigned char* fg = reinterpret_cast<unsigned char*>(s + p.fg);
    const bool vec4 = p.Ws % 4 == 0 && ((uintptr_t)j.count.y & 15) == 0;
    hipLaunchKernelGGL(vec4 ? unwarp_fg_kernel<true> : unwarp_fg_kernel<false>, dim3((unsigned)(p.B * p.cpi)), dim3(256), 0, stream, s + p.owner,
                       s + p.rowx, s + p.dec, j.count.y, fg, p.Hs, p.Ws, p.h * p.w, p.K, (int)p.cpi);
    FS_LAUNCH_CHECK();
    FS_TRY(surface_launch(p.sp, fg, j.hd.out, s + p.hds, p.B, p.Hs, p.Ws, j.hd.q, stream));
  }
  return FS_OK;
}

}  // namespace

extern "C" {

int fs_inverse_index_maps(const float* grid, long long* u, long long* v, long n, int H, int W, hipStream_t stream) {
  FS_REQUIRE(grid && u && v && n > 0 && H > 0 && W > 0);
  hipLaunchKernelGGL(inverse_index_kernel, dim3(cdiv(n, 256)), dim3(256), 0, stream, grid, u, v, n, H, W);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

int fs_inverse_grid(const float* grid, int* owner, float* grid_inv, int B, int h, int w, int Hs, int Ws, hipStream_t stream) {
  FS_REQUIRE(grid && owner && grid_inv && B > 0 && h > 0 && w > 0 && Hs > 0 && Ws > 0 && (long)h * w < INT_LIMIT);
  const long n = (long)B * Hs * Ws;
  FS_TRY(claim_owners(grid, owner, B, h, w, Hs, Ws, stream));
  hipLaunchKernelGGL(inverse_grid_kernel, dim3(cdiv(n, 256)), dim3(256), 0, stream, owner, grid_inv, n, h, w);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

int fs_fill_nearest(float* vals, const int* owner, int* scratch, int B, int C, int Hs, int Ws, hipStream_t stream) {
  FS_REQUIRE(vals && owner && scratch && B > 0 && C > 0 && Hs > 0 && Ws > 0 && (long)Hs * Ws < INT_LIMIT && row_fits_lds(Ws));
  const long per = (long)Hs * Ws, n = (long)B * per;
  int* rowx = scratch;          // [B*Hs*Ws]
  int* src = scratch + n;       // [B*Hs*Ws]
  FS_TRY(row_nearest_launch(owner, rowx, B, Hs, Ws, stream));
  hipLaunchKernelGGL(fill_col_nearest_kernel, dim3(cdiv(n, 256)), dim3(256), 0, stream, rowx, src, n, Hs, Ws);
  FS_LAUNCH_CHECK();
  hipLaunchKernelGGL(fill_copy_kernel, dim3(cdiv(n, 256)), dim3(256), 0, stream, vals, owner, src, C, per, n);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

// include/fovealseg.h: ints of scratch each entry point needs = the total of the plan for its feature set (0 for an empty shape)
long fs_unwarp_labels_scratch_ints(int B, int h, int w, int Hs, int Ws) { return unwarp_plan(B, 2, h, w, Hs, Ws, UW_LABELS).total; }
long fs_unwarp_accuracy_scratch_ints(int B, int h, int w, int Hs, int Ws) { return unwarp_plan(B, 2, h, w, Hs, Ws, UW_COUNT).total; }
long fs_unwarp_trimap_scratch_ints(int B, int h, int w, int Hs, int Ws) { return unwarp_plan(B, 2, h, w, Hs, Ws, UW_COUNT | UW_TRIM).total; }
long fs_unwarp_class_areas_scratch_ints(int B, int K, int h, int w, int Hs, int Ws) {
  return unwarp_plan(B, K, h, w, Hs, Ws, UW_COUNT | UW_AREA).total;
}
long fs_trimap_bands_scratch_ints(int B, int Hs, int Ws) { return trimap_plan(B, Hs, Ws).ints; }
// the layout with every other feature's regions: a call without areas or trimap needs less
long fs_unwarp_hd_scratch_ints(int B, int K, int h, int w, int Hs, int Ws) {
  return unwarp_plan(B, K, h, w, Hs, Ws, UW_COUNT | UW_AREA | UW_HD).total;
}
long fs_surface_hd_scratch_ints(int B, int Hs, int Ws) { return surface_plan(B, Hs, Ws).total; }

int fs_unwarp_labels(const float* cls, const float* m, const float* grid, long long* labels, unsigned char* hole, int* scratch, int B, int K,
                     int h, int w, int Hs, int Ws, hipStream_t stream) {
  return unwarp_run(unwarp_plan(B, K, h, w, Hs, Ws, UW_LABELS), {cls, m, grid, scratch, {labels, hole}}, stream);
}

int fs_unwarp_accuracy(const float* cls, const float* m, const float* grid, const float* y, const long long* cls_label, long long* counts,
                       float* acc, long long* labels, int* scratch, int B, int K, int h, int w, int Hs, int Ws, hipStream_t stream) {
  return unwarp_run(unwarp_plan(B, K, h, w, Hs, Ws, UW_COUNT), {cls, m, grid, scratch, {labels}, {y, cls_label, counts, acc}}, stream);
}

int fs_trimap_bands(const float* y, unsigned char* band, int* scratch, int B, int Hs, int Ws, int D, int frame, hipStream_t stream) {
  const TrimapPlan t = trimap_plan(B, Hs, Ws);
  FS_REQUIRE(y && band && scratch && t.ok && trimap_args_ok(D, frame));
  return trimap_launch(t, y, band, reinterpret_cast<unsigned char*>(scratch), B, Hs, Ws, D, frame, stream);
}

int fs_unwarp_trimap(const float* cls, const float* m, const float* grid, const float* y, const long long* cls_label, long long* counts,
                     float* acc, long long* trim, long long* labels, int* scratch, int B, int K, int h, int w, int Hs, int Ws, int D, int frame,
                     hipStream_t stream) {
  return unwarp_run(unwarp_plan(B, K, h, w, Hs, Ws, UW_COUNT | UW_TRIM),
                    {cls, m, grid, scratch, {labels}, {y, cls_label, counts, acc}, {trim, D, frame}}, stream);
}

// trim == nullptr: no trimap, D and frame are not read
int fs_unwarp_class_areas(const float* cls, const float* m, const float* grid, const float* y, const long long* cls_label, long long* counts,
                          float* acc, long long* areas, long long* trim, long long* labels, int* scratch, int B, int K, int h, int w, int Hs,
                          int Ws, int D, int frame, hipStream_t stream) {
  return unwarp_run(unwarp_plan(B, K, h, w, Hs, Ws, UW_COUNT | UW_AREA | (trim ? UW_TRIM : 0)),
                    {cls, m, grid, scratch, {labels}, {y, cls_label, counts, acc}, {trim, D, frame}, {areas}}, stream);
}

// areas == nullptr: no class areas; trim == nullptr: no trimap, D and frame are not read
int fs_unwarp_hd(const float* cls, const float* m, const float* grid, const float* y, const long long* cls_label, long long* counts, float* acc,
                 long long* areas, long long* trim, long long* labels, long long* hd, int* scratch, int B, int K, int h, int w, int Hs, int Ws,
                 int D, int frame, int q, hipStream_t stream) {
  return unwarp_run(unwarp_plan(B, K, h, w, Hs, Ws, UW_COUNT | UW_HD | (areas ? UW_AREA : 0) | (trim ? UW_TRIM : 0)),
                    {cls, m, grid, scratch, {labels}, {y, cls_label, counts, acc}, {trim, D, frame}, {areas}, {hd, q}}, stream);
}

long fs_unwarp_instances_scratch_ints(int B, int h, int w, int Hs, int Ws) { return unwarp_plan(B, 2, h, w, Hs, Ws, UW_BITS).total; }
int fs_unwarp_instances(const float* cls, const float* m, const float* grid, long long* cat, long long* stats, int* counts, unsigned int* bits,
                        int* scratch, int B, int K, int h, int w, int Hs, int Ws, int cap, hipStream_t stream) {
  return unwarp_run(unwarp_plan(B, K, h, w, Hs, Ws, UW_BITS), {cls, m, grid, scratch, {}, {}, {}, {}, {}, {cat, stats, counts, bits, cap}}, stream);
}

// the per-grid-point foreground probabilities alone: the table without the flag
int fs_head_fg_q(const float* cls, const float* m, int* q, int B, int K, int h, int w, hipStream_t stream) {
  FS_REQUIRE(cls && m && q && B > 0 && h > 0 && w > 0 && K >= 2 && K <= UNWARP_MAX_K && (long)h * w < INT_LIMIT);
  const long bpi = ((long)h * w + 1 + 255) / 256;
  FS_REQUIRE((long)B * bpi * 256 <= THREADS_MAX);
  hipLaunchKernelGGL(head_fg_q_kernel, dim3((unsigned)(B * bpi)), dim3(256), 0, stream, cls, m, (const int*)nullptr, q, K, h, w, (int)bpi);
  FS_LAUNCH_CHECK();
  return FS_OK;
}

long fs_unwarp_instances_scored_scratch_ints(int B, int h, int w, int Hs, int Ws) {
  return unwarp_plan(B, 2, h, w, Hs, Ws, UW_BITS | UW_SCORE).total;
}
int fs_unwarp_instances_scored(const float* cls, const float* m, const float* grid, long long* cat, long long* stats, int* counts,
                               unsigned int* bits, float* conf, long long* qsum, int* scratch, int B, int K, int h, int w, int Hs, int Ws,
                               int cap, hipStream_t stream) {
  return unwarp_run(unwarp_plan(B, K, h, w, Hs, Ws, UW_BITS | UW_SCORE),
                    {cls, m, grid, scratch, {}, {}, {}, {}, {}, {cat, stats, counts, bits, cap, conf, qsum}}, stream);
}

// the scratch of the scored call, which holds the unscored one's; conf == nullptr (with qsum): no score
long fs_unwarp_instances_component_scratch_ints(int B, int h, int w, int Hs, int Ws) {
  return unwarp_plan(B, 2, h, w, Hs, Ws, UW_BITS | UW_SCORE | UW_COMP).total;
}
int fs_unwarp_instances_component(const float* cls, const float* m, const float* grid, const float* focus, long long* cat, long long* stats,
                                  int* counts, unsigned int* bits, long long* comp, float* conf, long long* qsum, int* scratch, int B, int K,
                                  int h, int w, int Hs, int Ws, int cap, int conn, long snap2, hipStream_t stream) {
  FS_REQUIRE((conf == nullptr) == (qsum == nullptr));
  return unwarp_run(unwarp_plan(B, K, h, w, Hs, Ws, UW_BITS | UW_COMP | (conf ? UW_SCORE : 0u)),
                    {cls, m, grid, scratch, {}, {}, {}, {}, {}, {cat, stats, counts, bits, cap, conf, qsum}, {focus, comp, conn, snap2}}, stream);
}

int fs_surface_hd(const unsigned char* fg, long long* hd, int* scratch, int B, int Hs, int Ws, int q, hipStream_t stream) {
  const SurfacePlan sp = surface_plan(B, Hs, Ws);
  FS_REQUIRE(fg && hd && scratch && ((uintptr_t)scratch & 15) == 0 && sp.ok && hd_args_ok(q));
  return surface_launch(sp, fg, hd, scratch, B, Hs, Ws, q, stream);
}

}  // extern "C"
