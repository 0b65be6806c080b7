/* fovealseg.h -- C ABI of libfovealseg_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary of the FovealSeg forward/backward hot path.  The reference has no FFI: every op on
 * this path is an ATen call made from Python (models/models.py:666-1094 and the modules it drives).
 * Each entry point below replaces one such call (or a fixed group of them); the citation after each
 * prototype names the reference call site it stands in for (paths relative to the reference root).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer into memory owned by the caller (PyTorch caching allocator);
 *     the library never allocates, frees or synchronises;
 *   - activations are NHWC fp32 (B,H,W,C) unless a prototype says NCHW; conv weights are RSCK
 *     ([R][S][Cin][Cout]) -- the physical layout behind the reference's logical (Cout,Cin,R,S) shape;
 *   - `stream` is a hipStream_t passed as void*; kernels are enqueued on it and return immediately;
 *   - return value: 0 on success, 1001 (FS_ERR_ARG) for a rejected shape/pointer, otherwise the
 *     hipError_t of the failed launch.  Nothing is launched when an argument is rejected.
 *   - ACT codes: 0 none, 1 ReLU, 2 ReLU6.
 */
#ifndef FOVEALSEG_H
#define FOVEALSEG_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef void* fs_stream_t;

/* ---- foveation front-end ------------------------------------------------------------------ */
/* Input pipeline step in front of the path: one decoded sample, uint8 on the device, becomes slot b of the
 * float batch.  img (H,W,Ci) uint8 in PIL memory order ('RGBA': Ci=4, 'RGB': 3); X (B,Cx,HP,WP) with Cx <= Ci leading channels,
 * X = img/255 (transforms.ToTensor) zero-padded by (left,right,top,bottom) (F.pad); mask (H,W) uint8 -> Y (B,1,HP,WP) float,
 * same padding (Y / mask nullable).  Bit-identical to DynamicFocus/e_preprocess_scripts/dataset.py:127-142 + default collate,
 * at a quarter of the H2D bytes. */
int fs_ingest_sample(const unsigned char* img, const unsigned char* mask, float* X, float* Y, int b, int H, int W, int Ci, int Cx,
                     int pad_left, int pad_right, int pad_top, int pad_bottom, fs_stream_t stream);
/* x (B,3,H,W) NCHW, focus (B,2)=(row,col) -> out (B,hs,ws,5): bilinear RGB + 2x squared gaze distance.
 * models/models.py:684-705 (gen_grid_mtx_2xHxW, sqrt/square, b_imresize, 2x cat). */
int fs_gaze_lowres_fwd(const float* x, const float* focus, float* out, int B, int H, int W, int hs, int ws, fs_stream_t stream);
/* CompressNet.forward on its own: s (B,HW,C) -> out (B,HW) = w . relu(s) + bias (the logits; C <= 32), and its backward
 * (ds, dw (C), db (1) overwritten).  models/models.py:360-372 (the plugin contract net_compress((B,24,.,.)) -> (B,1,.,.), call site :713). */
int fs_compress_fwd(const float* s, const float* w, const float* bias, float* out, int B, int HW, int C, fs_stream_t stream);
/* scratch (both backward entry points): B*(C+1) floats -- the per-image partial sums of dw and db, added in image order (every
 * cross-workgroup sum of this library is two launches, partials then an ordered sum: no result depends on workgroup timing). */
int fs_compress_bwd(const float* g, const float* s, const float* w, float* ds, float* dw, float* db, int B, int HW, int C,
                    float* scratch, fs_stream_t stream);
/* s (B,HW,C) -> xs (B,HW) = softmax_HW(w . relu(s) + bias), HW <= 16384 (one workgroup keeps an image's logits in LDS; the launcher
 * asks for the 64 KiB of dynamic LDS the largest map needs), C <= 32.  models/models.py:369-372,715-723. */
int fs_compress_softmax_fwd(const float* s, const float* w, const float* bias, float* xs, int B, int HW, int C, fs_stream_t stream);
/* backward: C a multiple of 4; scratch = fs_compress_softmax_bwd_scratch_floats(B, C) floats (round 5: eight workgroups per image, one
 * record of C + 1 partial sums each). */
long fs_compress_softmax_bwd_scratch_floats(int B, int C);
int fs_compress_softmax_bwd(const float* g, const float* xs, const float* s, const float* w, float* ds, float* dw, float* db,
                            int B, int HW, int C, float* scratch, fs_stream_t stream);
/* y (B,1,H,W) -> (B,1,hs,ws) adaptive area average.  models/models.py:730. */
int fs_area_pool_fwd(const float* y, float* out, int B, int H, int W, int hs, int ws, fs_stream_t stream);
/* loss = coef * mean((minmax(xs) - minmax(t))^2) with whole-batch min/max.  stats = fs_edge_loss_stats_floats(n) floats, 32-byte
 * aligned, kept for bwd: [xs_min, xs_max, t_min, t_max, n_argmin, n_argmax] followed by the per-workgroup partial records of both
 * passes (round 5: every pass over the batch runs on up to 256 workgroups; whole-batch statistics are partials + an ordered sum).
 * models/models.py:889-891,898 (coef = 0.05 * edge_loss_scale). */
long fs_edge_loss_stats_floats(long n);
int fs_edge_loss_fwd(const float* xs, const float* t, long n, float coef, float* loss, float* stats, fs_stream_t stream);
int fs_edge_loss_bwd(const float* xs, const float* t, long n, float coef, const float* gout, float* stats, float* dxs,
                     fs_stream_t stream);
/* xs (B,hs,ws) -> grid (B,hs,ws,2)=(x,y) in [-1,1]: replication pad + Gaussian-weighted centroid + clamp.
 * g1d = the 2*pad+1 separable Gaussian taps (double).  models/models.py:594-637,819-821. */
int fs_gauss_grid_fwd(const float* xs, const double* g1d, float* grid, int B, int hs, int ws, int pad, fs_stream_t stream);
/* backward: scratch = fs_gauss_grid_bwd_scratch_floats(B, hs, ws) floats (round 5: four workgroups per image, each a band of grid columns;
 * the first of two launches hands (dp, dax, day) per grid point to the second). */
long fs_gauss_grid_bwd_scratch_floats(int B, int hs, int ws);
int fs_gauss_grid_bwd(const float* xs, const double* g1d, const float* dgrid, float* dxs, int B, int hs, int ws, int pad,
                      float* scratch, fs_stream_t stream);
/* The same pair under the other two settings of TRAIN.def_saliency_pad_mode (models/models.py:819-825): pad_mode 0 = 'replication'
 * (nn.ReplicationPad2d, what the two entry points above run), 1 = 'reflect' (F.pad(mode='reflect'); FS_ERR_ARG when pad > side - 1, which
 * torch refuses too), 2 = 'zero' (F.pad(mode='constant')).  The padded map is never materialised in any mode. */
int fs_gauss_grid_fwd_mode(const float* xs, const double* g1d, float* grid, int B, int hs, int ws, int pad, int pad_mode,
                           fs_stream_t stream);
int fs_gauss_grid_bwd_mode(const float* xs, const double* g1d, const float* dgrid, float* dxs, int B, int hs, int ws, int pad,
                           int pad_mode, float* scratch, fs_stream_t stream);
/* nn.Upsample(size=(H,W), mode='bilinear') of the deformation grid, align_corners=False: grid (B,h,w,2) -> out (B,H,W,2); the
 * task network may run at a higher resolution than the saliency map (TRAIN.task_input_size != saliency_input_size).
 * The backward needs integer factors H/h, W/w.  models/models.py:621-631. */
int fs_grid_upsample_fwd(const float* grid, float* out, int B, int h, int w, int H, int W, fs_stream_t stream);
int fs_grid_upsample_bwd(const float* g, float* dgrid, int B, int h, int w, int H, int W, fs_stream_t stream);
/* F.grid_sample(x, grid): bilinear / zeros / align_corners=False, bit-exact with ATen-CPU.
 * x (B,C,H,W) NCHW; out (B,h,w,C) if nhwc_out else (B,C,h,w).  models/models.py:909. */
int fs_grid_sample_fwd(const float* x, const float* grid, float* out, int B, int C, int H, int W, int h, int w, int nhwc_out,
                       fs_stream_t stream);
/* label = trunc(F.grid_sample(y, grid)) as int64; ysamp (nullable) gets the float sample.  models/models.py:880,951. */
int fs_grid_sample_label(const float* y, const float* grid, long long* label, float* ysamp, int B, int H, int W, int h, int w,
                         fs_stream_t stream);
/* autograd of grid_sample w.r.t. grid / w.r.t. input (scatter-add, dx overwritten). */
int fs_grid_sample_bwd_grid(const float* gout, const float* x, const float* grid, float* dgrid, int B, int C, int H, int W, int h,
                            int w, int nhwc, fs_stream_t stream);
int fs_grid_sample_bwd_input(const float* gout, const float* grid, float* dx, int B, int C, int H, int W, int h, int w, int nhwc,
                             fs_stream_t stream);
/* Inverse (un-foveating) warp, SURVEY §8(f)-3.  fs_inverse_grid: owner[b,v,u] = index yi*w+xi of the grid point that claims
 * full-resolution pixel (v,u) (-1 = hole; duplicates: the largest index wins, as ATen-CPU index_put_ does), grid_inv[b,v,u] =
 * (xi/w*2-1, yi/h*2-1), 0 in holes: feed it to fs_grid_sample_fwd(pred, grid_inv).  models/models.py:639-655,930-934.
 * fs_fill_nearest: every hole of vals (B,C,Hs,Ws) takes the value of the Euclidean-nearest claimed pixel (ties: smallest row,
 * then column) -- fillMissingValues_tensor(..., interp_mode='nearest'), models/models.py:159-286.  scratch = 2*B*Hs*Ws ints. */
int fs_inverse_grid(const float* grid, int* owner, float* grid_inv, int B, int h, int w, int Hs, int Ws, fs_stream_t stream);
int fs_fill_nearest(float* vals, const int* owner, int* scratch, int B, int C, int Hs, int Ws, fs_stream_t stream);
/* Full-resolution class map of the C1 head without the (B,K,Hs,Ws) prediction: labels (B,Hs,Ws) int64 is bit-identical to
 * argmax over k of fs_fill_nearest(fs_grid_sample_fwd(fs_pred_assemble_fwd(cls, m), grid_inv)) (first maximal k; NaN is maximal),
 * the route of models/models.py:639-655,930-940 followed by the eval caller's torch.max(scores, dim=1) (eval.py:195).  Every
 * pixel's K values are one grid point's samples (its owner's, its nearest claimed pixel's owner's, (0,0) in an image without a
 * claim), so the argmax is taken once per grid point and gathered.  cls (B,K), m (B,h,w) at the grid's resolution, grid (B,h,w,2);
 * hole (B,Hs,Ws) bytes, nullable: 1 where no grid point claims the pixel.  scratch = fs_unwarp_labels_scratch_ints(B, h, w, Hs, Ws)
 * ints.  FS_ERR_ARG for K < 2 or K > 1024, Ws > 16384, or sizes beyond 32-bit pixel indices. */
long fs_unwarp_labels_scratch_ints(int B, int h, int w, int Hs, int Ws);
int fs_unwarp_labels(const float* cls, const float* m, const float* grid, long long* labels, unsigned char* hole, int* scratch, int B, int K,
                     int h, int w, int Hs, int Ws, fs_stream_t stream);
/* The four full-resolution accuracies of MODEL.upsample (models/models.py:378-474,869-873,1074-1083) without the class map: the
 * predicted class of pixel (b,v,u) is fs_unwarp_labels' (same kernels up to the gather), its ground truth is t = (long)y[b,v,u],
 * gt = t * cls_label[b] + (1 - t) * (K - 1) (:968), and the gather pass counts instead of storing.  y (B,Hs,Ws) fp32 label mask,
 * cls_label (B) int64.  counts (B,6) int64 = cls_fg, bin_fg, union_fg, cls_bg, bin_bg, union_bg per image, background = K - 1, as
 * fs_seg_loss_fwd counts them; acc (4) = acc, acc_bin_fg, acc_cls_fbg, acc_bin_fbg in its arithmetic (fp32 quotients with 1e-10
 * added to the unions, summed over the images in a fixed order, / B).  labels (B,Hs,Ws) int64, nullable: fs_unwarp_labels' map.
 * Counts are integer sums of per-workgroup records (plain stores, no atomics, scratch not zeroed): bit-reproducible in every mode.
 * scratch = fs_unwarp_accuracy_scratch_ints(B, h, w, Hs, Ws) ints, 16-byte aligned.  FS_ERR_ARG as fs_unwarp_labels, and for
 * Hs * Ws within 1024 (one workgroup's pixels) of 2^31. */
long fs_unwarp_accuracy_scratch_ints(int B, int h, int w, int Hs, int Ws);
int fs_unwarp_accuracy(const float* cls, const float* m, const float* grid, const float* y, const long long* cls_label,
                       long long* counts, float* acc, long long* labels, int* scratch, int B, int K, int h, int w, int Hs, int Ws,
                       fs_stream_t stream);
/* Trimap bands (eval.py:41-67, trim_accuracy): band (B,Hs,Ws) bytes = for every pixel the smallest i <= D such that the pixel lies
 * within 2^i city-block steps of the label's boundary, 255 if none -- the reference's FIND_EDGES + binary_dilation(iterations=2**i)
 * masks, i = 0 .. D, as one map.  y (B,Hs,Ws) fp32 label mask, t = (long)y.  A seed is a background pixel (t == 0) with a foreground
 * (t != 0) 8-neighbour, pixels outside the image being background; frame = 1 also makes every background pixel of the outer one-pixel
 * ring a seed, as PIL's filter does (the reference bit for bit), frame = 0 is the neighbour rule alone.  Exact: two separable passes
 * of capped L1 distances.  scratch = fs_trimap_bands_scratch_ints(B, Hs, Ws) ints.  FS_ERR_ARG for a null pointer, D outside 0..7,
 * frame outside {0, 1}, non-positive sizes. */
long fs_trimap_bands_scratch_ints(int B, int Hs, int Ws);
int fs_trimap_bands(const float* y, unsigned char* band, int* scratch, int B, int Hs, int Ws, int D, int frame, fs_stream_t stream);
/* fs_unwarp_accuracy with the trimap boundary accuracies of eval.py:41-67 counted in the same gather pass: counts, acc and labels
 * are fs_unwarp_accuracy's bit for bit; trim (B,D+1,3) int64 = per image and band i (fs_trimap_bands of y, made here): the pixels in
 * the band, those whose predicted class equals gt (the reference's acc_sum), those that agree with gt on foreground versus
 * background.  An image without a seed (constant label with frame = 0, all foreground with frame = 1) has all-zero rows, where the
 * reference divides 0 by 0.  Integer sums of per-workgroup records, as counts.  scratch = fs_unwarp_trimap_scratch_ints(B, h, w,
 * Hs, Ws) ints, 16-byte aligned.  FS_ERR_ARG as fs_unwarp_accuracy and fs_trimap_bands, and for a null trim. */
long fs_unwarp_trimap_scratch_ints(int B, int h, int w, int Hs, int Ws);
int fs_unwarp_trimap(const float* cls, const float* m, const float* grid, const float* y, const long long* cls_label, long long* counts,
                     float* acc, long long* trim, long long* labels, int* scratch, int B, int K, int h, int w, int Hs, int Ws, int D,
                     int frame, fs_stream_t stream);
/* fs_unwarp_accuracy with the per-class areas of the reference's evaluation summary (eval.py:218-257,313-322; utils.py:289-317,
 * intersectionAndUnion with ignore_index = none) counted in the same gather pass.  areas (B,3,K,3) int64: per image, space and class
 * k the triple (inter, pred, lab) = #(a == k and g == k), #(a == k), #(g == k) of a class map a against its ground truth g; the
 * union is pred + lab - inter (utils.py:312), left to the caller.  Space 0: a = fs_unwarp_labels' class, g = t*cls_label + (1-t)*(K-1),
 * t = (long)y, over the Hs*Ws pixels.  Space 1, the sampling ceiling (VAL.y_sampled_reverse, "intrinsic upsampling error IoU(Y', Y)",
 * models/models_instance.py:909-918): a = gs[q] of the grid point q that feeds the pixel, gs[p] = ts*cls_label + (1-ts)*(K-1) with
 * ts = (long)bilinear(y, grid[p]), fs_grid_sample_label's value bit for bit, against the same g; background in an image without a
 * claimed pixel.  It is the label of the feeding point itself, NOT the reference's F.grid_sample(mode='nearest') at the inverse
 * coordinate: that coordinate is xi - 0.5 up to fp32 rounding, a round-half-to-even tie decided by rounding noise.  Space 2, the
 * sampled space: a = first maximal k of the low-resolution prediction at grid point p (cls[b,k] for k < K-1, cls[b,K-1] * m[b,p],
 * one rounded multiply; NaN maximal, as torch.max, eval.py:197), g = gs[p], over the h*w points.  Rows are defined by equality: a
 * cls_label outside 0 .. K-1 has no lab / inter row (np.histogram's range drops it), cls_label == K-1 merges into the background
 * row.  y reads as 0 or 1 after truncation; other values are not defined.  counts, acc and labels are fs_unwarp_accuracy's bit for
 * bit.  trim nullable: given, it is fs_unwarp_trimap's bit for bit (bands made here, D and frame as there); null, D and frame are
 * ignored.  Integer sums throughout: the two hot classes (cls_label, K-1) in per-workgroup records, every other predicted class
 * through an LDS histogram and 32-bit integer atomics into a zeroed (B,K) table of sums in scratch; bit-reproducible.  scratch =
 * fs_unwarp_class_areas_scratch_ints(B, K, h, w, Hs, Ws) ints, 16-byte aligned.  FS_ERR_ARG as fs_unwarp_accuracy (and
 * fs_unwarp_trimap with trim), and for a null areas. */
long fs_unwarp_class_areas_scratch_ints(int B, int K, int h, int w, int Hs, int Ws);
int fs_unwarp_class_areas(const float* cls, const float* m, const float* grid, const float* y, const long long* cls_label,
                          long long* counts, float* acc, long long* areas, long long* trim, long long* labels, int* scratch,
                          int B, int K, int h, int w, int Hs, int Ws, int D, int frame, fs_stream_t stream);
/* Surface distance between two masks: the q-th percentile of the Hausdorff distances (HD95 at q = 95; VAL.hd95, utils.py:25-101), as
 * the integers it is made of.  fg (B,Hs,Ws) bytes, any alignment: bit 0 = foreground of the first mask (the prediction), bit 1 = of
 * the second (the label).  The border of a mask is its foreground with a background 4-neighbour, everything outside the image
 * counting as background (foreground XOR binary_erosion by the cross); every border pixel of one mask takes the squared Euclidean
 * distance d^2 to the nearest border pixel of the other, in both directions, and the two sets are pooled: n = n_pred + n_label
 * integers.  hd (B,4) int64 = (n_pred, n_label, d2_lo, d2_hi): the pooled values of ranks lo = q (n-1) div 100 and hi = lo + (q (n-1)
 * mod 100 != 0) in ascending order -- np.percentile(., q) is sqrt(d2_lo) + (sqrt(d2_hi) - sqrt(d2_lo)) * (q (n-1) mod 100) / 100 --
 * and d2_lo = d2_hi = -1 where either border is empty.  This is the published 2-D definition, NOT what utils.hd95 returns: that
 * function flattens both masks to 1-D before it erodes them, and nothing in the reference calls it.  Exact: a column pass (vertical
 * distance to the nearest border pixel), a row pass (the exact minimum over the row, pruned once dx^2 alone reaches the best value), a
 * two-level radix select over integer histograms with the row pass run once per level; no list of distances, integer atomics only,
 * bit-reproducible.  q = 1 .. 100.  scratch = fs_surface_hd_scratch_ints(B, Hs, Ws) ints, 16-byte aligned.  FS_ERR_ARG, with nothing
 * launched, for a null pointer, a misaligned scratch, q outside 1 .. 100, non-positive sizes, Hs > 16384 or Ws > 16384. */
long fs_surface_hd_scratch_ints(int B, int Hs, int Ws);
int fs_surface_hd(const unsigned char* fg, long long* hd, int* scratch, int B, int Hs, int Ws, int q, fs_stream_t stream);
/* fs_unwarp_class_areas with fs_surface_hd of the prediction against the label behind the count pass: hd (B,4) int64 as there, the
 * first mask being "fs_unwarp_labels' class is not K-1" and the second t = (long)y != 0, gathered into a byte map in scratch (no
 * (B,Hs,Ws) class map exists).  areas, trim and labels are nullable: given, each is fs_unwarp_class_areas' bit for bit; counts and acc
 * are fs_unwarp_accuracy's.  scratch = fs_unwarp_hd_scratch_ints(B, K, h, w, Hs, Ws) ints, 16-byte aligned (>= the class areas').
 * FS_ERR_ARG as fs_unwarp_class_areas for what is given, as fs_surface_hd, and for a null hd. */
long fs_unwarp_hd_scratch_ints(int B, int K, int h, int w, int Hs, int Ws);
int fs_unwarp_hd(const float* cls, const float* m, const float* grid, const float* y, const long long* cls_label, long long* counts,
                 float* acc, long long* areas, long long* trim, long long* labels, long long* hd, int* scratch, int B, int K, int h, int w,
                 int Hs, int Ws, int D, int frame, int q, fs_stream_t stream);
/* A byte mask as bit words.  mask (B,Hs,Ws) bytes, any alignment, non-zero = foreground; bits (B,Hs,P) 32-bit words, P =
 * ceil(Ws / 32): bit j of word i of row y is pixel x = 32 i + j, bits at x >= Ws are 0.  FS_ERR_ARG for a null pointer, non-positive
 * sizes or more than 2^32 - 256 bit slots (B * Hs * P * 32). */
int fs_mask_bits(const unsigned char* mask, unsigned int* bits, int B, int Hs, int Ws, fs_stream_t stream);
/* Area, box and uncompressed COCO run-length code of a bit mask, exact and on the device (the format is restated from its published
 * definition; the reference has no RLE code).  bits (B,Hs,P) as fs_mask_bits makes them.  The mask is flattened column-major, v[p],
 * p = x * Hs + y, N = Hs * Ws, v[-1] = 0; the boundaries are T = {p : v[p] != v[p-1]} ascending, and the code is T[0], T[i] - T[i-1],
 * N - T[last]: the first count is the leading run of zeros (0 when pixel (0,0) is set), runs continue from the bottom of a column into
 * the top of the next, an empty mask gives [N], a full one [0, N].  stats (B,6) int64 = (area, x0, y0, bw, bh, n_runs): the set
 * pixels, their box [x0, y0, bw, bh] (all 0 for an empty mask) and n_runs = |T| + 1, always the true number.  counts (B,cap) int32:
 * the first min(n_runs, cap) entries are the code's, every later entry is 0; n_runs > cap tells a truncated code, nothing is written
 * past cap.  Three passes over (column, 64-row segment) items in column-major order -- count the boundaries of an item, scan the
 * counts per image, walk again and store -- plain stores only, no atomics, no host read: the same bits in every mode.  scratch =
 * fs_mask_rle_scratch_ints(B, Hs, Ws) ints.  FS_ERR_ARG, with nothing launched, for a null pointer, cap < 1, non-positive sizes or
 * Hs * Ws >= 2^31. */
long fs_mask_rle_scratch_ints(int B, int Hs, int Ws);
int fs_mask_rle(const unsigned int* bits, long long* stats, int* counts, int* scratch, int B, int Hs, int Ws, int cap, fs_stream_t stream);
/* fs_mask_rle's inverse: the uncompressed run-length code back into bit words, exact and on the device (UNPINNED, as the code itself).
 * counts (B,cap) int32 as fs_mask_rle defines them: runs of 0, 1, 0, ... over the mask flattened column-major, p = x * Hs + y, the run
 * of zeros first.  n_runs[b * n_stride] int64 = the length of image b's code: a (B) vector has n_stride = 1, a stats (B,6) tensor is
 * passed as it lies (pointer to its column 5, n_stride = 6).  Entries of counts at or past n_runs are never read.  Every well-formed
 * code is accepted, canonical or not: zero-length runs may stand anywhere, [N] is the empty mask and [0, N] the full one, N = Hs * Ws.
 * With end[r] the sum of the first r + 1 counts, pixel p takes (the first r with end[r] > p) & 1.  bits (B,Hs,P), P = ceil(Ws/32), in
 * fs_mask_bits' layout, the bits at x >= Ws always 0; every word is written by a plain store: nothing to zero beforehand, no atomics,
 * no host read, the same bits in every mode.  info (B,4) int64 = (status, area, n_read, total): n_read = min(max(n_runs, 0), cap);
 * total = the int64 sum of the n_read counts; status = the first that applies of 1 CUT (n_runs > cap), 2 BAD (n_runs < 1, or a count
 * read is negative), 3 SUM (total != N), else 0; area = the sum of the odd-indexed counts where status is 0, else 0.  An image whose
 * status is not 0 gets all-zero words; no code makes the kernels read or write outside their tensors (every address comes from B, Hs,
 * Ws, cap and n_read alone).  Two passes: one workgroup an image scans the counts into clamped int ends in scratch and writes info; a
 * wave per 64 columns x 64 rows bisects for the run of each column's first pixel, walks down the columns and ballots a row's two
 * words.  scratch = fs_rle_bits_scratch_ints(B, cap) ints (B * cap + 2 B; 0 for B < 1 or cap < 1), any 4-byte alignment; its contents
 * after the call are unspecified.  FS_ERR_ARG, with nothing launched, for a null pointer, n_stride < 1, cap < 1, non-positive sizes,
 * Hs * Ws >= 2^31 or more than 2^32 - 256 bit slots (B * Hs * P * 32). */
long fs_rle_bits_scratch_ints(int B, int cap);
int fs_rle_bits(const int* counts, const long long* n_runs, int n_stride, unsigned int* bits, long long* info, int* scratch, int B, int Hs,
                int Ws, int cap, fs_stream_t stream);
/* COCO / LVIS polygon lists into bit words, exact and on the device.  The reference makes its labels this way in its dataset
 * preparation (DynamicFocus/e_preprocess_scripts/b2_preprocess_lvis.py:282-297): per polygon np.round, a clip of x to [0, W-1] and of y
 * to [0, H-1], skimage.draw.polygon, and the union of the polygons as the label.  UNPINNED: skimage is not at hand, so the definition
 * is this library's, restated from that call site -- what skimage.draw.polygon is understood to produce for integer vertices (the
 * interior plus the edge and vertex points), not verified against it.  It is NOT pycocotools' frPoly, which traces a 5x upsampled
 * outline and differs along the rim.
 *   vertex  (vy, vx) = (clamp(y, 0, Hs-1), clamp(x, 0, Ws-1)); the caller rounds (round half to even on the file's double), the
 *           kernel clamps: any int32 is defined and no vertex value ever forms an address.
 *   ring    the closed chain of a polygon's n >= 1 vertices, edges (v_i, v_(i+1) mod n).
 *   pixel   the integer point (y, x) is set by a ring iff (a) it lies on an edge, end points included (cross product 0 and inside the
 *           edge's box; a one-vertex ring is its point, a two-vertex ring its segment's lattice points), or (b) the crossing number is
 *           odd: of the edges oriented so that y0 < y1 with y0 <= y < y1, those with (x - x0)(y1 - y0) < (y - y0)(x1 - x0) are
 *           counted; horizontal edges do not count.
 *   mask    the OR of the image's rings: overlapping polygons do not cancel, a self-intersecting ring follows even-odd.
 * verts (V,2) int32 = (y, x), rounded, not clipped; ring_off (R+1) int32: ring r owns verts[ring_off[r] : ring_off[r+1]]; img_ring
 * (B+1) int32: image b owns the rings img_ring[b] : img_ring[b+1]; vertices no ring of the call's images owns are never read.  bits
 * (B,Hs,P), P = ceil(Ws/32), in fs_mask_bits' layout, the bits at x >= Ws always 0; every word is written by a plain store: nothing to
 * zero beforehand, no atomics on global memory, no host read.  info (B,4) int64 = (status, area, n_rings, n_vertices): status 1 where
 * img_ring[b], img_ring[b+1] are not 0 <= . <= . <= R or, over the image's rings, ring_off[r], ring_off[r+1] are not 0 <= . <= . <= V
 * -- such an image gets all-zero words and (1, 0, 0, 0); else 0, area = the set pixels, n_rings and n_vertices as the offsets say.  An
 * image without rings, or with empty rings only, is the empty mask with status 0.  One workgroup per image and band of
 * fs_poly_bits_band_rows(Hs, Ws) = min(Hs, 64, 4096 / P) rows keeps a toggle buffer and the mask in LDS (32 KiB at the most) and takes
 * ring after ring: every non-horizontal edge flips, for each of its rows y0 <= y < y1 in the band, the bit at column x0 + ceil((y -
 * y0)(x1 - x0) / (y1 - y0)) (exact, by an incremental division) and ORs in its lattice points, horizontal edges OR their span; a
 * prefix-XOR along each toggled row is the even-odd interior.  XOR and OR in LDS do not depend on order: the same bits in every mode
 * and every run.  scratch = fs_poly_bits_scratch_ints(B, Hs, Ws) ints (one popcount per image and band, summed into info by a second
 * kernel; 0 for sizes that are refused), any 4-byte alignment, as verts and bits.  FS_ERR_ARG, with nothing launched, for a null
 * pointer, non-positive B, Hs or Ws, negative R or V, a side above 16384 (every product of two coordinate differences stays inside
 * int32), Hs * Ws >= 2^31 or more than 2^32 - 256 bit slots (B * Hs * P * 32). */
long fs_poly_bits_scratch_ints(int B, int Hs, int Ws);
int fs_poly_bits_band_rows(int Hs, int Ws);
int fs_poly_bits(const int* verts, const int* ring_off, const int* img_ring, unsigned int* bits, long long* info, int* scratch, int B, int R,
                 int V, int Hs, int Ws, fs_stream_t stream);
/* The gazed instance of the C1 head as a record, without a class map: the mask is "fs_unwarp_labels' class is not K-1" bit for bit
 * (same kernels up to the gather, which stores bit words instead of classes), stats and counts are fs_mask_rle's of it.  cat (B)
 * int64 = the first maximal k < K-1 of cls[b,k], NaN maximal (torch.argmax(cls[:, :K-1], 1)): the head's classification, and the
 * class of every set pixel except where the bilinear sample of that constant plane ties two classes by rounding or has no in-bounds
 * weight.  bits (B,Hs,P) as fs_mask_bits', nullable: null keeps the words in scratch.  scratch =
 * fs_unwarp_instances_scratch_ints(B, h, w, Hs, Ws) ints; 16-byte aligned, four pixels a thread are gathered where Ws % 4 == 0.
 * FS_ERR_ARG as fs_unwarp_labels and fs_mask_rle, and for a null cat. */
long fs_unwarp_instances_scratch_ints(int B, int h, int w, int Hs, int Ws);
int fs_unwarp_instances(const float* cls, const float* m, const float* grid, long long* cat, long long* stats, int* counts,
                        unsigned int* bits, int* scratch, int B, int K, int h, int w, int Hs, int Ws, int cap, fs_stream_t stream);
/* The foreground probability of the C1 head per grid point, as an integer (no counterpart in the reference: UNPINNED, a definition of
 * this library's).  v[b,:,p] = the K fp32 values that the bilinear sample of the prediction (fs_pred_assemble_fwd's) holds at grid point
 * p's inverse coordinate, p < h*w, and at (0,0) for p = h*w -- the values fs_unwarp_labels takes the argmax of, formed by the same
 * float operations.  P = sum_{k<K-1} exp(v_k - max v) / sum_{k<K} exp(v_k - max v), evaluated in fp64 from the fp32 v: the softmax mass
 * of the classes below K-1.  q (B, h*w+1) int32 = rint(P * 2^24), 0 .. 2^24; 0 where P is NaN (a NaN or +inf among the v, or every v
 * -inf).  FS_ERR_ARG for a null pointer, non-positive sizes, K < 2 or K > 1024. */
int fs_head_fg_q(const float* cls, const float* m, int* q, int B, int K, int h, int w, fs_stream_t stream);
/* fs_unwarp_instances with a confidence for the record (UNPINNED, as the run-length code): cat, stats, counts and bits are
 * fs_unwarp_instances' bit for bit.  qsum (B) int64 = the sum of fs_head_fg_q's q[b, feeding point] over the set pixels of the mask,
 * added in the gather that stores the bit words; below 2^55, and an integer sum: the same bits in every order and precision mode.
 * conf (B,3) fp32 = (score, cls_prob, mask_prob): mask_prob = qsum / (area * 2^24) formed in fp64, 0 for an empty mask; cls_prob =
 * the fp64 softmax over cls[b, :K-1] at cat[b], NaN where that row holds a NaN; score = the fp64 product of the two; each rounded to
 * fp32 once.  Where no tap of a set pixel's sample lies out of bounds, P * cls_prob is the K-way softmax probability of class cat
 * there: score is the mean probability of the predicted class over the predicted mask.  Every wave of the gather stores the sum of
 * its first image as a record, summed per image in a fixed pass; only a wave that straddles two images adds the second one's part
 * with a 64-bit integer atomic.  scratch = fs_unwarp_instances_scored_scratch_ints(B, h, w, Hs, Ws) ints >= the unscored query, by the
 * table's B * (h*w+1) ints, the records (a quarter of an int per bit word where Ws % 4 == 0, half of one otherwise) and alignment: less than a bit a pixel.  FS_ERR_ARG, with nothing launched, as fs_unwarp_instances, and for a null conf or
 * qsum. */
long fs_unwarp_instances_scored_scratch_ints(int B, int h, int w, int Hs, int Ws);
int fs_unwarp_instances_scored(const float* cls, const float* m, const float* grid, long long* cat, long long* stats, int* counts,
                               unsigned int* bits, float* conf, long long* qsum, int* scratch, int B, int K, int h, int w, int Hs,
                               int Ws, int cap, fs_stream_t stream);
/* The connected component of a mask under the gaze (no counterpart in the reference: UNPINNED, a definition of this library's;
 * DESIGN.md §1 f-3).  All integers, on bit words.  bits (B,Hs,P), P = ceil(Ws/32), as fs_mask_bits lays them out (the bits at x >= Ws
 * are not read as pixels); focus (B,2) fp32 = normalised (row, col); conn = 4 (edge neighbours) or 8 (edge and corner neighbours);
 * snap2 = a squared distance in whole pixels.  The gaze pixel is fs_gate_decide's: gy = clamp(rint((double)f_row * ((Hs-1) * 16)), 0,
 * (Hs-1) * 16), NaN -> 0, py = (gy + 8) >> 4, px likewise with Ws.  The seed is (py, px) where that bit is set (d2 = 0), else the set
 * pixel (y, x) that minimises key = d2 * 2^31 + (y * Ws + x), d2 = (y-py)^2 + (x-px)^2: the nearest set pixel, ties to the smaller
 * row-major index.  There is no component for an empty mask or where d2 > snap2.  The component is every set pixel joined to the seed
 * by a path of set pixels with steps of the chosen neighbourhood; outside the image is background.  out (B,Hs,P) = its bit words, all 0
 * where there is none, the bits at x >= Ws always 0; out may not be bits.  comp (B,4) int64 = (seed_y, seed_x, d2, area_all), area_all
 * the popcount of the input within x < Ws; (-1, -1, -1, area_all) where there is no component.  A set function of the input: the same
 * bits in every order of execution.  One workgroup per image grows the reached set until a sweep adds nothing; the set lives in LDS
 * where Hs * (P | 1) words fit 156 KiB (fs_mask_component_route = 1), in out itself otherwise (= 2; 0 for sizes that are refused).
 * scratch = fs_mask_component_scratch_ints(B, Hs, Ws) ints, any 4-byte alignment; its contents after the call are unspecified.  FS_ERR_ARG, with nothing launched, for a null
 * pointer, out == bits, conn outside {4, 8}, snap2 < 0, non-positive sizes, a side above 16384 or Hs * Ws >= 2^31. */
long fs_mask_component_scratch_ints(int B, int Hs, int Ws);
int fs_mask_component_route(int B, int Hs, int Ws);
int fs_mask_component(const unsigned int* bits, const float* focus, unsigned int* out, long long* comp, int* scratch, int B, int Hs,
                      int Ws, int conn, long snap2, fs_stream_t stream);
/* Erosion of a bit mask by a (2d+1) x (2d+1) square (no counterpart in the reference: UNPINNED, restated from the published definition
 * of Boundary IoU, Cheng et al., CVPR 2021: copyMakeBorder(0) + erode(3x3, iterations = d)).  All integers, on bit
 * words.  bits (B,Hs,P), P = ceil(Ws/32), as fs_mask_bits lays them out (the bits at x >= Ws are not read as pixels).  out (B,Hs,P):
 * bit (y,x) is set iff every pixel of the square centred on (y,x) is set, every pixel outside the image counting as unset; the bits at
 * x >= Ws always 0; out may not be bits.  2d+1 above a side is legal and gives the empty erosion.  The boundary band of Boundary IoU is
 * bits & ~out.  A rows pass then a columns pass, each an AND over 2d+1 neighbours built by doubling in LDS (O(log d) steps), the plane
 * between them in scratch = fs_mask_erode_scratch_ints(B, Hs, Ws, d) ints (0 for sizes that are refused), any 4-byte alignment; its
 * contents after the call are unspecified.  FS_ERR_ARG, with nothing launched, for a null pointer, out == bits, non-positive sizes, a
 * side above 16384, Hs * Ws >= 2^31, d < 1 or d > 2047. */
long fs_mask_erode_scratch_ints(int B, int Hs, int Ws, int d);
int fs_mask_erode(const unsigned int* bits, unsigned int* out, int* scratch, int B, int Hs, int Ws, int d, fs_stream_t stream);
/* The counters of mask IoU and Boundary IoU of two bit masks (UNPINNED, as fs_mask_erode).  a, b (B,Hs,P) as fs_mask_bits lays them out
 * (the bits at x >= Ws are not read; a may be b).  With the band of a mask m, band(m) = m & ~E_d(m), E_d fs_mask_erode's, pair (B,6)
 * int64 = (|a & b|, |a|, |b|, |band(a) & band(b)|, |band(a)|, |band(b)|); with 2d+1 above a side the bands are the masks.  Both
 * erosions and the popcounts run with no host read in between; the popcounts are reduced by shuffles into one record a workgroup,
 * added per image in index order (no atomics: the same numbers in every order of execution).  scratch =
 * fs_mask_pair_scratch_ints(B, Hs, Ws, d) ints (four bit planes an image and the records; 0 for sizes that are refused), any 4-byte
 * alignment; its contents after the call are unspecified.  FS_ERR_ARG, with nothing launched, for a null pointer and as fs_mask_erode
 * for the sizes and d. */
long fs_mask_pair_scratch_ints(int B, int Hs, int Ws, int d);
int fs_mask_pair_counts(const unsigned int* a, const unsigned int* b, long long* pair, int* scratch, int B, int Hs, int Ws, int d,
                        fs_stream_t stream);
/* Of an image's annotated instances, the one under the gaze.  The reference builds its labels by choosing one annotation and putting
 * the gaze on a pixel inside it (DynamicFocus/e_preprocess_scripts/b2_preprocess_lvis.py:258-333: rasterise the annotation, ridx_rrcc =
 * np.random.randint(len(rrs))); this is the inverse of that step -- the gaze and the annotations are given, the annotation looked at is
 * asked for -- and has no counterpart there.  UNPINNED: the definition is this library's.  All integers, on bit
 * words.  cbits (N,Hs,P), P = ceil(Ws/32), the candidates' masks as fs_mask_bits lays them out (the bits at x >= Ws are not read as
 * pixels); cand_off (B+1) int32: image b owns the rows cand_off[b] .. cand_off[b+1]-1; cand_cat (N) int64 the rows' classes, nullable;
 * focus (B,2) fp32 = normalised (row, col); pbits (B,Hs,P) one prediction an image (the record's mask), nullable; snap2 = a squared
 * distance in whole pixels.  The gaze pixel (py, px) is fs_mask_component's: gy = clamp(rint((double)f_row * ((Hs-1) * 16)), 0, (Hs-1)
 * * 16), NaN -> 0, py = (gy + 8) >> 4, px likewise with Ws.  Per candidate n of image b: area = its set pixels; inter = |c_n & p_b| (0
 * without pbits); its nearest set pixel to the gaze = the minimum of key = d2 * 2^31 + (y * Ws + x), d2 = (y-py)^2 + (x-px)^2
 * (fs_mask_component's seed rule, ties to the smaller row-major index); cand (N,6) int64 = (b, area, inter, d2, near_y, near_x), the
 * last three -1 for an empty candidate.  The SELECTED instance of image b is, among its candidates with area > 0 and d2 <= snap2, the
 * least (d2, area, n) in lexicographic order: where several contain the gaze pixel the smallest one (a cup on a table gives the cup),
 * where none does the nearest one within the snap distance, ties to the smaller area, then the smaller row.  The BEST-OVERLAPPING
 * instance is, among candidates with inter > 0, the one of the greatest inter / (area + |p_b| - inter), compared exactly by
 * cross-multiplication in int64 (the products stay below 2^57), ties to the smaller area, then the smaller row.  sel (B,8) int64 =
 * (index, cls, d2, area, inter, n_hit, best, status): index the selected global row or -1; cls = cand_cat[index], -1 for no selection
 * or no cand_cat; d2, area, inter the selected row's (-1, 0, 0 for none); n_hit the number of the image's candidates that contain the
 * gaze pixel; best the best-overlapping row or -1; status 0.  gbits (B,Hs,P) = the selected candidate's words, the bits at x >= Ws 0;
 * all 0 where none is selected; every word is written by a plain store: nothing to zero beforehand.  cand_off is valid iff cand_off[0]
 * == 0, it is non-decreasing and cand_off[B] == N; otherwise every image gets status 1, index = best = -1, cls = d2 = -1, area = inter
 * = n_hit = 0 and zero gbits, and every cand row is (-1, area, 0, -1, -1, -1).  Validity is decided once, by a pass of its own, before
 * anything depends on it; a candidate finds its image by bisecting cand_off, so no offset value and no cand_cat value ever forms an
 * address (cand_cat is read at a selected row only).  N = 0 is valid: every image selects nothing (cbits and cand may then be null).
 * A workgroup per (candidate, band of at most 256 rows and 8192 words) reads the candidate's words once and writes one record (area,
 * inter, |p|, key) into scratch; a wave per image adds its candidates' records in index order and selects; a workgroup per (image,
 * band) copies.  No atomics, no host read: the same bits in every run.  scratch = fs_mask_candidates_scratch_ints(B, N, Hs, Ws) ints
 * (0 for sizes that are refused), any 4-byte alignment; its contents after the call are unspecified.  FS_ERR_ARG, with nothing
 * launched, for a null pointer other than cand_cat and pbits (and cbits, cand with N = 0), gbits == cbits, B < 1, N < 0, a side below 1
 * or above 16384, Hs * Ws >= 2^31, N or B times the bands an image beyond int range, snap2 < 0. */
long fs_mask_candidates_scratch_ints(int B, int N, int Hs, int Ws);
int fs_mask_candidates(const unsigned int* cbits, const int* cand_off, const long long* cand_cat, const float* focus,
                       const unsigned int* pbits, long long* cand, long long* sel, unsigned int* gbits, int* scratch, int B, int N, int Hs,
                       int Ws, long snap2, fs_stream_t stream);
/* fs_unwarp_instances / fs_unwarp_instances_scored with the record describing the component under the gaze instead of every foreground
 * pixel (no counterpart in the reference: UNPINNED).  The decide / owner / fill passes and the bit gather are fs_unwarp_instances';
 * with conf the gather is still the unscored one -- the words are the same, and the scored gather's sums over the whole mask would be
 * discarded -- and fs_head_fg_q's table is made beside it.  fs_mask_component's passes take the component of the gathered words
 * (focus, conn, snap2 and comp as there); fs_mask_rle's passes
 * run once, on the component's words.  stats, counts and bits (nullable) are the component's; cat is unchanged.  conf and qsum are
 * given or null together: qsum (B) = the sum of fs_head_fg_q's q over the set bits of the component only (the same owner / nearest
 * look-up and table read per bit as the scored gather; integer sums: one record per eight consecutive bit words by plain stores,
 * summed per image in a fixed pass, and only a group of eight that straddles an image's end adds the further image's part into qsum
 * with a 64-bit integer atomic, as the scored gather's straddling waves do), conf (B,3) as
 * fs_unwarp_instances_scored's with that qsum and the component's area: cls_prob is unchanged, mask_prob and score describe the
 * component.  With no component the record is the empty mask's: stats all 0 but n_runs = 1, the code [Hs * Ws], mask_prob = score =
 * 0.  No host read between the steps.  scratch = fs_unwarp_instances_component_scratch_ints(B, h, w, Hs, Ws) ints (the scored call's,
 * two bit planes' worth less one where bits is kept, and the component's).  FS_ERR_ARG, with nothing launched, as
 * fs_unwarp_instances_scored and fs_mask_component, and for conf and qsum not both given or both null. */
long fs_unwarp_instances_component_scratch_ints(int B, int h, int w, int Hs, int Ws);
int fs_unwarp_instances_component(const float* cls, const float* m, const float* grid, const float* focus, long long* cat,
                                  long long* stats, int* counts, unsigned int* bits, long long* comp, float* conf, long long* qsum,
                                  int* scratch, int B, int K, int h, int w, int Hs, int Ws, int cap, int conn, long snap2,
                                  fs_stream_t stream);
/* The gaze gate (no counterpart in the reference: UNPINNED, a definition of this library's): does the record a viewer
 * holds still answer for a new frame and gaze?  All integers.  Pixel code q(v) = (int) rintf(fminf(fmaxf(v, 0), 1) * 255.0f): one fp32
 * multiply, round to nearest even, NaN -> 0, k/255 -> k.  fs_gate_tiles, the hot pass: img (B,3,H,W) fp32 NCHW, the new frames; key
 * (B,3,H,W) bytes, q of the frame each viewer's record was made from; T in {8, 16, 32, 64}, th = ceil(H/T), tw = ceil(W/T), the last
 * tiles ragged.  sad (B,th,tw) int32 = the sum over the 3 channels and the tile's pixels of |q(img) - key|.  15 bytes read per pixel;
 * every entry is one workgroup's, written with a plain store: no atomics, nothing to zero.  Four pixels a lane (a 16-byte load of img, a
 * 4-byte load of key) where W % 4 == 0, img is 16-byte and key 4-byte aligned; one pixel a lane otherwise.  FS_ERR_ARG, with nothing
 * launched, for a null pointer, non-positive sizes, T outside the set, H * W >= 2^31 or more than 2^24 - 1 tiles. */
int fs_gate_tiles(const float* img, const unsigned char* key, int* sad, int B, int H, int W, int T, fs_stream_t stream);
/* The decision per viewer (UNPINNED).  sad as fs_gate_tiles makes it; gstate (B,6) int64 = (valid, gy_key, gx_key, gy_prev, gx_prev,
 * age); focus (B,2) fp32 = normalised (row, col); stats (B,6) int64 and bits (B,H,P) the record's, as fs_mask_rle / fs_mask_bits make
 * them; force (B) int32, nullable.  The gaze in 1/16-pixel units: gy = clamp(rint((double)f_row * ((H-1)*16)), 0, (H-1)*16), gx likewise
 * with W, NaN -> 0; the gaze pixel (py, px) = ((gy+8)>>4, (gx+8)>>4); d2 = the squared distance of two such points.  A tile is changed
 * iff sad > level * n_el, n_el = 3 * its true pixel count.  The region of interest is every tile that meets the box [x0, y0, bw, bh]
 * grown by margin pixels and clipped (nothing when area = 0), plus the tile of the gaze pixel.  The first rule that holds decides:
 *   7 RUN_FORCED force[b] != 0;  1 RUN_INIT valid == 0;  2 HOLD_SACCADE d2(g, g_prev) > saccade2;  3 RUN_SCENE n_changed > scene_tiles;
 *   4 RUN_ROI n_roi_changed > roi_tiles;  5 RUN_GAZE not (inside_on and the mask's bit at (py, px)) and d2(g, g_key) > fixation2;
 *   6 RUN_AGE max_age > 0 and age + 1 > max_age;  0 REUSE.
 * gate (B,8) int64 = (code, n_changed, n_roi_changed, sad_total, d2_key, d2_prev, inside_bit, age + 1), every column written for every
 * viewer.  One workgroup a viewer sums its tiles, one lane decides; nothing but gate is written.  The thresholds come squared, in
 * 1/16-pixel units: floor((px * 16)^2).  FS_ERR_ARG, with nothing launched, for a null pointer other than force, non-positive sizes, T
 * outside the set, level outside 0 .. 254, margin < 0, H * W >= 2^31, or a side above 2^26 (d2 stays below 2^62). */
int fs_gate_decide(const int* sad, const long long* gstate, const float* focus, const long long* stats, const unsigned int* bits,
                   const int* force, long long* gate, int B, int H, int W, int T, int level, int scene_tiles, int roi_tiles, int margin,
                   long saccade2, long fixation2, int max_age, int inside_on, fs_stream_t stream);
/* What a step leaves behind (UNPINNED).  idx (n) int32 ascending = the viewers whose record was made anew; row j of the src tensors
 * (cat (n), stats (n,6) int64, counts (n,cap) int32, bits (n,H,P), conf (n,3) fp32) belongs to viewer idx[j].  For those viewers key <-
 * q(img[idx[j]]) (img is the whole (B,3,H,W) batch), g_key <- g, age <- 0, valid <- 1, and the rows are copied j -> idx[j] into the dst
 * tensors of B rows.  For every viewer g_prev <- g; one that is not in idx gets age <- age + 1.  A pair with src == dst is already in
 * place and is not touched; conf is nullable, as a pair.  n == 0: the state pass alone is launched, idx may be null.  An idx entry
 * outside 0 .. B-1 writes nothing.  FS_ERR_ARG, with nothing launched, for a null pointer, non-positive sizes, cap < 1, n outside 0 ..
 * B, H * W >= 2^31 or a side above 2^26. */
int fs_gate_commit(const float* img, const int* idx, int n, unsigned char* key, long long* gstate, const float* focus,
                   const long long* src_cat, const long long* src_stats, const int* src_counts, const unsigned int* src_bits,
                   const float* src_conf, long long* dst_cat, long long* dst_stats, int* dst_counts, unsigned int* dst_bits,
                   float* dst_conf, int B, int H, int W, int cap, fs_stream_t stream);
/* Global motion compensation in front of the gate (no counterpart in the reference: UNPINNED, a definition of this library's; DESIGN.md
 * §1 f-3; its defaults are not validated on real gaze data): a viewer's record is carried along a camera that translates by whole
 * pixels, and the unchanged gate then verifies the move.  All integers.  The pixel code q is the gate's, NaN -> 0; the luma code is
 * L(y,x) = q_r + q_g + q_b, 0 .. 765.  Profiles: prof (B, H + W) int32, row b = [prow (H) | pcol (W)], prow[y] = sum_x L, pcol[x] =
 * sum_y L.  fs_frame_profiles takes img (B,3,H,W) fp32 NCHW, fs_key_profiles key (B,3,H,W) bytes: the profiles of a frame and of the key
 * commit made from it are equal.  The hot pass, 12 bytes a pixel: four pixels a lane by 16-byte (4-byte: key) loads where W % 4 == 0
 * and the pointer is so aligned, one pixel a lane otherwise; prof is zeroed, then row sums (shuffles) and column sums (lanes, LDS) are
 * added with integer atomics, so every order gives the same integers.  FS_ERR_ARG, with nothing launched, for a null pointer,
 * non-positive sizes, H * W >= 2^31 or 765 * max(H, W) >= 2^31. */
int fs_frame_profiles(const float* img, int* prof, int B, int H, int W, fs_stream_t stream);
int fs_key_profiles(const unsigned char* key, int* prof, int B, int H, int W, fs_stream_t stream);
/* The integer translation of every viewer (UNPINNED).  prof the new frames' profiles, prof_key the key frames'; gstate (B,6) the gate's.
 * Per axis, for a new profile P, a key profile K of length n and s in [-R, R]: cost(s) = sum_{i=R}^{n-1-R} |P[i] - K[i - s]| in int64
 * (the content at i came from i - s).  The best s has the least cost, ties going to the smaller |s|, then to the negative s; it is
 * taken only if cost(s) * 8 <= cost(0) * gain, gain 0 .. 8, and is 0 otherwise (sensor noise on a still camera must not walk the record
 * a pixel at a time).  shift (B,4) int64 = (dy, dx, cost_best, cost_zero): dy from prow, dx from pcol, cost_best the sum over the two
 * axes of the least cost (whether or not the gain rule took its shift), cost_zero of cost(0).  A viewer with valid == 0 gets (0, 0, 0,
 * 0).  One workgroup a viewer, both profiles of an axis and the 2R+1 costs in LDS.  FS_ERR_ARG, with nothing launched, as
 * fs_frame_profiles and unless 1 <= R <= 255, 4R < min(H, W), 0 <= gain <= 8 and 8 * max(H, W) + 8 * (2R+1) <= 65536 bytes of LDS. */
int fs_profile_shift(const int* prof, const int* prof_key, const long long* gstate, long long* shift, int B, int H, int W, int R, int gain,
                     fs_stream_t stream);
/* Move the state of every viewer whose (dy, dx) = shift[b, 0:2] is not (0, 0) (UNPINNED); a still viewer's tensors are not written and
 * cost no key traffic (every workgroup reads shift[b] and leaves).  img (B,3,H,W) fp32 the new frames.
 *   key'[c,y,x] = key[c,y-dy,x-dx] where that lies in the frame, else q(img[c,y,x]): the uncovered border cannot be judged and counts
 *     as unchanged.  bits'[y,x] = bits[y-dy,x-dx], else 0; the bits at x >= W are 0.
 *   gstate: gy_key, gy_prev += 16 dy and gx_key, gx_prev += 16 dx, clamped to [0, (side-1) * 16]: the previous gaze moves too, so a
 *     counter-rotating eye is not read as a saccade.  stats / counts become fs_mask_rle's of bits' (cap entries), through its passes.
 *   prof_key becomes the profiles of key'.  mstate (B,4) int64 = (dy_total, dx_total, moves, path) grows by (dy, dx, 1, |dy| + |dx|).
 * cat and conf are not touched: mask_prob keeps describing the pixels the record was made from.  For every viewer motion (B,6) int64 =
 * (dy, dx, cost_best, cost_zero, dy_total, dx_total), the totals after this move.  The move does not read what it writes: the moved
 * planes are written to key2 (B,3,H,W) and bits2 (B,H,P) and copied back (the bits by funnel shifts over the word borders, four key
 * bytes a lane where W % 4 == 0 and key, key2 are 4-byte aligned); the contents of key2, bits2 and scratch after the call are
 * unspecified.  scratch = fs_state_shift_scratch_ints(B, H, W, cap) ints, 8-byte aligned (0 for sizes that are refused).  FS_ERR_ARG,
 * with nothing launched, for a null pointer, key2 == key, bits2 == bits, a misaligned scratch, cap < 1, as fs_frame_profiles and
 * fs_mask_rle for the sizes, or a side above 2^26. */
long fs_state_shift_scratch_ints(int B, int H, int W, int cap);
int fs_state_shift(const float* img, const long long* shift, unsigned char* key, unsigned char* key2, unsigned int* bits,
                   unsigned int* bits2, long long* gstate, long long* stats, int* counts, int* prof_key, long long* mstate,
                   long long* motion, int* scratch, int B, int H, int W, int cap, fs_stream_t stream);
/* After fs_gate_commit (UNPINNED): for the viewers idx[0 .. n) whose record was made anew, prof_key <- prof (this step's frame
 * profiles: the profiles of the key frame commit made) and mstate <- 0.  n == 0 launches nothing, idx may be null; an idx entry outside
 * 0 .. B-1 writes nothing.  FS_ERR_ARG for a null pointer, n outside 0 .. B, and as fs_frame_profiles for the sizes. */
int fs_motion_commit(const int* idx, int n, const int* prof, int* prof_key, long long* mstate, int B, int H, int W, fs_stream_t stream);
/* Frames as bytes (no counterpart in the reference: UNPINNED).  A uint8 frame is planar (B,3,H,W) bytes, contiguous; its
 * pixel value is v = (float)byte / 255.0f, correctly rounded (fs_ingest_sample's expression), and its pixel code q(v) is the byte itself.
 * Each entry point below equals its fp32 twin fed byte / 255 bit for bit, and returns FS_ERR_ARG, with nothing launched, under the twin's
 * conditions.  The profiles of such a frame are fs_key_profiles of it.
 * fs_gaze_lowres_u8_fwd: fs_gaze_lowres_fwd with the four taps of every low-resolution point converted as they are read. */
int fs_gaze_lowres_u8_fwd(const unsigned char* x, const float* focus, float* out, int B, int H, int W, int hs, int ws, fs_stream_t stream);
/* fs_grid_sample_fwd on bytes, forward only: x (B,C,H,W) bytes, out fp32 (B,h,w,C) [nhwc_out=1] or (B,C,h,w) [nhwc_out=0]; the taps of
 * fs_grid_sample_fwd, an out-of-bounds tap 0.f, the same multiply and three fused multiply-adds. */
int fs_grid_sample_u8_fwd(const unsigned char* x, const float* grid, float* out, int B, int C, int H, int W, int h, int w, int nhwc_out,
                          fs_stream_t stream);
/* fs_gate_tiles on bytes, the hot pass: sad (B,th,tw) int32 = the sum over the 3 channels and the tile's pixels of |img - key|, 6 bytes read
 * per pixel, plain stores, no atomics.  Sixteen pixels a lane (one 16-byte load of img and of key per channel, four v_sad_u8 each) where
 * W % 16 == 0 and both pointers are 16-byte aligned: a row takes the least power of two of lanes that covers min(W, 1024) columns and a
 * tile, so a wave of a narrow frame takes several rows at once; one pixel a lane otherwise. */
int fs_gate_tiles_u8(const unsigned char* img, const unsigned char* key, int* sad, int B, int H, int W, int T, fs_stream_t stream);
/* fs_gate_commit on bytes: key[idx[j]] <- img[idx[j]], a copy (sixteen bytes a lane where 3 * H * W % 16 == 0 and both pointers are 16-byte
 * aligned); the state and row passes are fs_gate_commit's. */
int fs_gate_commit_u8(const unsigned char* img, const int* idx, int n, unsigned char* key, long long* gstate, const float* focus,
                      const long long* src_cat, const long long* src_stats, const int* src_counts, const unsigned int* src_bits,
                      const float* src_conf, long long* dst_cat, long long* dst_stats, int* dst_counts, unsigned int* dst_bits,
                      float* dst_conf, int B, int H, int W, int cap, fs_stream_t stream);
/* fs_state_shift on bytes: the key's uncovered border is filled with the frame's byte; every other pass is fs_state_shift's, with the
 * same scratch (fs_state_shift_scratch_ints). */
int fs_state_shift_u8(const unsigned char* img, const long long* shift, unsigned char* key, unsigned char* key2, unsigned int* bits,
                      unsigned int* bits2, long long* gstate, long long* stats, int* counts, int* prof_key, long long* mstate,
                      long long* motion, int* scratch, int B, int H, int W, int cap, fs_stream_t stream);
/* Frames as interleaved bytes, read where they lie (UNPINNED): what cameras, decoders, OpenCV, PIL and numpy make.  The
 * frame is described by (img, sb, sy, sx): the byte of channel c at (b, y, x) is img[b * sb + y * sy + x * sx + c], c = 0 .. 2; sx = 3
 * (RGB) or 4 (RGBA / RGBX: the fourth byte reaches no result); a row spans W * sx bytes of a pitch sy >= W * sx; images lie sb >= H * sy
 * apart, or sb = 0: every viewer sees the one image.  Each entry point below equals its planar twin fed the de-interleaved frame bit for
 * bit, never writes the frame, and returns FS_ERR_ARG, with nothing launched, under the twin's conditions and for sx outside {3, 4}, sy <
 * W * sx, sb < 0, or 0 < sb < H * sy with B > 1.  The session's state stays planar.
 * fs_byte_frame_route (host only): which forms the passes take for such a frame of width W: 1 the vector forms (W % 16 == 0 and img, sy, sb
 * multiples of 16, so that every sixteen pixels of every row start at a 16-byte boundary), 0 the one-pixel forms (any width, pitch and
 * alignment), -1 a description that is refused (null img, sx, sy < W * sx, sb < 0, W < 1). */
long fs_byte_frame_route(const unsigned char* img, long sb, long sy, int sx, int W);
/* fs_gaze_lowres_u8_fwd on an interleaved frame: the same four taps and the same operations, a tap's three bytes from one address. */
int fs_gaze_lowres_hwc_fwd(const unsigned char* img, long sb, long sy, int sx, const float* focus, float* out, int B, int H, int W, int hs,
                           int ws, fs_stream_t stream);
/* fs_grid_sample_u8_fwd with C = 3 on an interleaved frame: out fp32 (B,h,w,3) [nhwc_out=1] or (B,3,h,w) [nhwc_out=0]; one address a tap
 * instead of three planes. */
int fs_grid_sample_hwc_fwd(const unsigned char* img, long sb, long sy, int sx, const float* grid, float* out, int B, int H, int W, int h, int w,
                           int nhwc_out, fs_stream_t stream);
/* fs_gate_tiles_u8 on an interleaved frame, the hot pass: 6 (sx = 3) or 7 (sx = 4) bytes read per pixel, plain stores, no atomics.  Vector
 * form (route 1 and key 16-byte aligned): fs_gate_tiles_u8's cut; a lane owns the 48 or 64 frame bytes of its sixteen pixels (three or
 * four 16-byte loads), splits them into a register quad a channel with v_perm_b32 (6 perms four RGB pixels, 7 four RGBA pixels) and meets
 * the key's 16-byte load per channel with v_sad_u8.  One pixel a lane otherwise. */
int fs_gate_tiles_hwc(const unsigned char* img, long sb, long sy, int sx, const unsigned char* key, int* sad, int B, int H, int W, int T,
                      fs_stream_t stream);
/* fs_gate_commit_u8 on an interleaved frame: key[idx[j]] <- the de-interleaved frame of viewer idx[j]; the key stays planar.  Sixteen
 * pixels a lane (split as in the tile pass, three 16-byte stores) under the tile pass's conditions, one byte a lane otherwise.  The state
 * and row passes are fs_gate_commit's. */
int fs_gate_commit_hwc(const unsigned char* img, long sb, long sy, int sx, const int* idx, int n, unsigned char* key, long long* gstate,
                       const float* focus, const long long* src_cat, const long long* src_stats, const int* src_counts,
                       const unsigned int* src_bits, const float* src_conf, long long* dst_cat, long long* dst_stats, int* dst_counts,
                       unsigned int* dst_bits, float* dst_conf, int B, int H, int W, int cap, fs_stream_t stream);
/* fs_key_profiles of an interleaved frame: prof (B, H + W) int32, the row and column sums of r + g + b per pixel.  Four pixels a lane (12
 * bytes in three 4-byte loads, or one 16-byte load) on route 1, one pixel a lane otherwise; the same zeroing and integer atomics. */
int fs_frame_profiles_hwc(const unsigned char* img, long sb, long sy, int sx, int* prof, int B, int H, int W, fs_stream_t stream);
/* fs_state_shift_u8 on an interleaved frame: only the move pass reads the frame (the key's uncovered border takes the frame's byte of
 * that channel); every other pass and the scratch are fs_state_shift's. */
int fs_state_shift_hwc(const unsigned char* img, long sb, long sy, int sx, const long long* shift, unsigned char* key, unsigned char* key2,
                       unsigned int* bits, unsigned int* bits2, long long* gstate, long long* stats, int* counts, int* prof_key,
                       long long* mstate, long long* motion, int* scratch, int B, int H, int W, int cap, fs_stream_t stream);
/* Frames as NV12, read where they lie (UNPINNED: the reference reads image files only): what a video decoder's surface
 * ("Y plane followed by interleaved UV plane", a device pointer and a pitch per plane), a camera ISP and V4L2 make.  1.5 bytes a pixel.
 * Layout.  A frame of B images of H x W pixels, any H, W >= 1, odd included, is (yp, uvp, sb, sy, ub, uy): the luma byte of (b, y, x) is
 * yp[b * sb + y * sy + x], sy >= W; with j = y >> 1, i = x >> 1 its chroma is U = uvp[b * ub + j * uy + 2 * i], V = uvp[b * ub + j * uy + 2 * i
 * + 1], uy >= 2 * ceil(W / 2): the sample of the pixel's 2 x 2 block, nearest, replicated -- no interpolation, no siting offset.  Images do
 * not overlap (sb >= H * sy, ub >= ceil(H / 2) * uy) or are all one image (sb = ub = 0); neither is looked at for B = 1.
 * Colour.  csc = (yo, yg, rv, gu, gv, bu), six int32 passed by value.  With C = Y - yo, D = U - 128, E = V - 128 in int32 and >> the
 * arithmetic (floor) shift:
 *   R = clamp((yg * C + rv * E          + 128) >> 8, 0, 255)
 *   G = clamp((yg * C + gu * D + gv * E + 128) >> 8, 0, 255)
 *   B = clamp((yg * C + bu * D          + 128) >> 8, 0, 255)
 * 0 <= yo <= 255 and every coefficient in [-32768, 32768], so no sum leaves int32.  The standard tables are rint(256 * real coefficient)
 * from (Kr, Kb), luma gain 255 / 219 and chroma gain 255 / 224 for limited range, 1 for full range (yo, yg, rv, gu, gv, bu):
 *   bt601 limited 16 298 409 -100 -208 516    bt601 full 0 256 359 -88 -183 454
 *   bt709 limited 16 298 459  -55 -136 541    bt709 full 0 256 403 -48 -120 475
 * each within 1 grey level of clip(rint(real formula)) over all 2^24 (Y, U, V).
 * The RGB byte is the pixel's code q and byte / 255 its value: each entry point below equals its planar uint8 twin fed fs_nv12_to_rgb's
 * planar frame bit for bit.  All integer work but the taps' (float)byte / 255; plain vector loads and stores; the frame is never written; no
 * address is formed from frame data.  FS_ERR_ARG, with nothing launched, under the twin's conditions and for a null plane, sy < W, uy < 2 *
 * ceil(W / 2), sb < 0, ub < 0, overlapping images with B > 1 (sb = 0 with ub != 0 among them), yo outside 0 .. 255 or a coefficient
 * outside [-32768, 32768].
 * fs_nv12_frame_route (host only): 1 the vector forms (W % 16 == 0, yp and uvp 16-byte aligned, sy, sb, uy, ub multiples of 16: every
 * sixteen pixels of a row and their sixteen chroma bytes are one aligned load each), 0 the one-pixel forms, -1 a description refused. */
long fs_nv12_frame_route(const unsigned char* yp, const unsigned char* uvp, long sb, long sy, long ub, long uy, int W);
/* The conversion alone: out, described as fs_frame_overlay's destination (planar, RGB, or RGBA with alpha 255), <- the RGB bytes.  Sixteen
 * pixels a lane (a 16-byte load of luma and one of chroma, the chroma products made once a sample) on route 1 with the destination's
 * sixteen-pixel pieces aligned, one pixel a lane otherwise.  What a caller displays, and the twin the other entry points are held to.
 * Also FS_ERR_ARG for out == yp or out == uvp. */
int fs_nv12_to_rgb(const unsigned char* yp, const unsigned char* uvp, long sb, long sy, long ub, long uy, int yo, int yg, int rv, int gu, int gv,
                   int bu, unsigned char* out, long ob, long oy, int ox, int B, int H, int W, fs_stream_t stream);
/* fs_gaze_lowres_u8_fwd on an NV12 frame: the same four taps, each converted as it is read, then the same operations. */
int fs_gaze_lowres_nv12_fwd(const unsigned char* yp, const unsigned char* uvp, long sb, long sy, long ub, long uy, int yo, int yg, int rv, int gu,
                            int gv, int bu, const float* focus, float* out, int B, int H, int W, int hs, int ws, fs_stream_t stream);
/* fs_grid_sample_u8_fwd with C = 3 on an NV12 frame: out fp32 (B,h,w,3) [nhwc_out=1] or (B,3,h,w) [nhwc_out=0]. */
int fs_grid_sample_nv12_fwd(const unsigned char* yp, const unsigned char* uvp, long sb, long sy, long ub, long uy, int yo, int yg, int rv, int gu,
                            int gv, int bu, const float* grid, float* out, int B, int H, int W, int h, int w, int nhwc_out, fs_stream_t stream);
/* fs_gate_tiles_u8 on an NV12 frame, the hot pass: 4.5 bytes read per pixel (1.5 of the frame, 3 of the key), plain stores, no atomics.
 * Vector form (route 1 and key 16-byte aligned): fs_gate_tiles_u8's cut; a lane converts its sixteen pixels into a register quad a
 * channel and meets the key's 16-byte load per channel with the same twelve v_sad_u8.  One pixel a lane otherwise. */
int fs_gate_tiles_nv12(const unsigned char* yp, const unsigned char* uvp, long sb, long sy, long ub, long uy, int yo, int yg, int rv, int gu, int gv,
                       int bu, const unsigned char* key, int* sad, int B, int H, int W, int T, fs_stream_t stream);
/* fs_gate_commit_u8 on an NV12 frame: key[idx[j]] <- the converted frame of viewer idx[j]; the key stays planar RGB bytes.  Sixteen
 * pixels a lane (three 16-byte stores) under the tile pass's conditions, one byte a lane otherwise. */
int fs_gate_commit_nv12(const unsigned char* yp, const unsigned char* uvp, long sb, long sy, long ub, long uy, int yo, int yg, int rv, int gu, int gv,
                        int bu, const int* idx, int n, unsigned char* key, long long* gstate, const float* focus, const long long* src_cat,
                        const long long* src_stats, const int* src_counts, const unsigned int* src_bits, const float* src_conf,
                        long long* dst_cat, long long* dst_stats, int* dst_counts, unsigned int* dst_bits, float* dst_conf, int B, int H, int W,
                        int cap, fs_stream_t stream);
/* fs_key_profiles of an NV12 frame: the row and column sums of the luma code r + g + b of the converted pixel, as everywhere -- not of
 * the Y plane.  Four pixels a lane (a 4-byte load of luma and one of chroma) on route 1, one pixel a lane otherwise. */
int fs_frame_profiles_nv12(const unsigned char* yp, const unsigned char* uvp, long sb, long sy, long ub, long uy, int yo, int yg, int rv, int gu,
                           int gv, int bu, int* prof, int B, int H, int W, fs_stream_t stream);
/* fs_state_shift_u8 on an NV12 frame: only the move pass reads the frame (the key's uncovered border takes the converted pixel's byte of
 * that channel); every other pass and the scratch are fs_state_shift's. */
int fs_state_shift_nv12(const unsigned char* yp, const unsigned char* uvp, long sb, long sy, long ub, long uy, int yo, int yg, int rv, int gu, int gv,
                        int bu, const long long* shift, unsigned char* key, unsigned char* key2, unsigned int* bits, unsigned int* bits2,
                        long long* gstate, long long* stats, int* counts, int* prof_key, long long* mstate, long long* motion, int* scratch,
                        int B, int H, int W, int cap, fs_stream_t stream);
/* Showing the record: the gazed instance drawn onto the frame (UNPINNED, a definition of this library's).  The reference
 * visualises on the host, with matplotlib, PIL and numpy (eval.py:70-83 visualize_result, utils.py:207-221 colorEncode, the TensorBoard
 * panels of models/models.py); this replaces what a caller composed from torch shifts, torch.where, an fp32 blend and permute().contiguous().
 * All integers.  For viewer b and pixel (y, x), s_c = the source pixel's code in channel c (fs_gate_tiles' q of an fp32 value, the byte
 * itself of a byte source); out_c is the first of these that applies:
 *   1 marker   r > 0, d2 = (y-py)^2 + (x-px)^2 <= r^2 and d2 >= max(r - w, 0)^2 -> the marker colour; (py, px) is fs_mask_component's gaze
 *              pixel (1/16-pixel units, NaN -> 0, clamped); w >= r gives a disc, a smaller w a ring.
 *   2 box      t > 0, the record's box (x0, y0, bw, bh) = stats[b, 1:5] has bw > 0, bh > 0 and contains (y, x), and x - x0 < t, x0 + bw - 1 -
 *              x < t, y - y0 < t or y0 + bh - 1 - y < t (within t pixels of a side, measured inward) -> the box colour.  The stats values
 *              are compared as integers only and never form an address: any int64 is defined, the sums taken without overflow.
 *   3 outline  the outline flag is on and the pixel's bit in band is set -> the outline colour.
 *   4 mask     the pixel's bit in bits is set -> (s_c * (256 - a) + tint_c * a + 128) >> 8.
 *   5 else     (s_c * dim + 128) >> 8: dim = 256 leaves the pixel as it is, a smaller dim darkens what the viewer does not look at.
 * bits, band (B,H,P), P = ceil(W/32), as fs_mask_bits lays them out (the bits at x >= W are never read as pixels); band is meant to be
 * bits & ~E_d(bits), E_d fs_mask_erode's, and is only read.  band, stats and focus are nullable: a null one switches its element off.
 * live is nullable, int64, read as live[b * live_stride]: where it is 0 the viewer's mask, band and box count as empty, the marker and
 * dim still apply (GazeSession passes column 0 of its gstate (B,6) as it lies, live_stride = 6).  style (S,20) int32 on the device, S = 1
 * (every viewer) or S = B (a row a viewer): columns 0-2 tint r g b, 3 a, 4-6 outline r g b, 7 dim, 8-10 box r g b, 11 t, 12-14 marker r g
 * b, 15 r, 16 w, 17 the outline flag, 18-19 reserved; every entry is clamped by the kernel (colours to 0 .. 255, a and dim to 0 .. 256, t,
 * r, w to 0 .. 16384) and none forms an address.
 * The destination is always bytes, (out, ob, oy, ox): ox = 1 planar, the byte of channel c at (b, y, x) is out[b * ob + c * H * W + y * W + x],
 * oy == W, ob >= 3 * H * W; ox = 3 or 4 interleaved, out[b * ob + y * oy + x * ox + c], oy >= W * ox, ob >= H * oy, and for ox = 4 the fourth
 * byte is written as 255 (ob is not looked at for B = 1).  One launch; every output byte is written once by a plain store: no atomics, no
 * host read, nothing to zero; the source is never written unless it is out.  out == img is allowed where source and destination have the
 * same description (planar bytes both, or equal sb, sy, sx): each workgroup reads its pixels before it stores them, and owns them alone.
 * fs_frame_overlay: img (B,3,H,W) fp32 NCHW, 12 bytes read and 3 or 4 written a pixel; sixteen pixels a lane (twelve 16-byte loads)
 * where W % 16 == 0, img is 16-byte aligned and the destination's pieces are as fs_frame_overlay_u8 asks, one otherwise.  FS_ERR_ARG, with nothing
 * launched, for a null img, bits, style or out, S outside {1, B}, non-positive sizes, a side above 16384, H * W >= 2^31, ox outside {1, 3,
 * 4}, a pitch or image step too small (ob = 0 with B > 1 among them), out == img with differing descriptions, live_stride < 1 with live
 * given. */
int fs_frame_overlay(const float* img, const unsigned int* bits, const unsigned int* band, const long long* stats, const float* focus,
                     const long long* live, long live_stride, const int* style, int S, unsigned char* out, long ob, long oy, int ox, int B,
                     int H, int W, fs_stream_t stream);
/* fs_frame_overlay on planar bytes (B,3,H,W).  Sixteen pixels a lane where W % 16 == 0, img is 16-byte aligned and the destination's
 * sixteen-pixel pieces are (out, oy and ob multiples of 16): three 16-byte loads, a half word of bits and of band, and three 16-byte
 * stores for a planar destination, or the sixteen pixels re-interleaved with v_perm_b32 (6 perms four RGB pixels, 8 four RGBA pixels) into
 * three or four 16-byte pieces, which a workgroup lays down in LDS in memory order so that neighbouring lanes store neighbouring
 * pieces.  One pixel a lane otherwise. */
int fs_frame_overlay_u8(const unsigned char* img, const unsigned int* bits, const unsigned int* band, const long long* stats,
                        const float* focus, const long long* live, long live_stride, const int* style, int S, unsigned char* out, long ob,
                        long oy, int ox, int B, int H, int W, fs_stream_t stream);
/* fs_frame_overlay_u8 on an interleaved frame (img, sb, sy, sx), read where it lies; also FS_ERR_ARG for a description fs_gate_tiles_hwc
 * refuses.  Sixteen pixels a lane on route 1 of fs_byte_frame_route and a destination as above: the lane's 48 or 64 bytes are split into
 * planar order in registers as fs_gate_tiles_hwc splits them, and joined again for an interleaved destination -- camera RGBA in, display
 * RGBA out is 4 bytes read and 4 written a pixel.  One pixel a lane otherwise. */
int fs_frame_overlay_hwc(const unsigned char* img, long sb, long sy, int sx, const unsigned int* bits, const unsigned int* band,
                         const long long* stats, const float* focus, const long long* live, long live_stride, const int* style, int S,
                         unsigned char* out, long ob, long oy, int ox, int B, int H, int W, fs_stream_t stream);
/* fs_frame_overlay_u8 on an NV12 frame ("frames as NV12" above), read where it lies: s_c is the converted pixel's byte; the destinations as
 * above, never the frame itself: FS_ERR_ARG for out == yp or out == uvp (no destination has the frame's description); that out overlaps
 * neither plane otherwise is the caller's duty, as for every entry point.  Sixteen pixels a lane on route 1 of fs_nv12_frame_route and a
 * destination as above, one otherwise. */
int fs_frame_overlay_nv12(const unsigned char* yp, const unsigned char* uvp, long sb, long sy, long ub, long uy, int yo, int yg, int rv, int gu,
                          int gv, int bu, const unsigned int* bits, const unsigned int* band, const long long* stats, const float* focus,
                          const long long* live, long live_stride, const int* style, int S, unsigned char* out, long ob, long oy, int ox,
                          int B, int H, int W, fs_stream_t stream);
/* A class map as colours: utils.py:207-221 colorEncode(labelmap, colors, mode='RGB') for fs_unwarp_labels' map.  labels (B,H,W) int64,
 * palette (K,3) bytes; out, described as fs_frame_overlay's destination, = palette[label], (0, 0, 0) for a label < 0 or >= K.  The
 * reference skips negative labels, which leaves its zeros, and would raise an IndexError on a label >= K: black there is this library's
 * choice.  A label forms an address only inside the palette.  Sixteen labels a lane where the destination's sixteen-pixel pieces and
 * labels are 16-byte aligned, one otherwise; plain stores, the same writer.  FS_ERR_ARG, with nothing launched, for a null pointer, K < 1,
 * and as fs_frame_overlay for the sizes and the destination. */
int fs_color_encode(const long long* labels, const unsigned char* palette, unsigned char* out, long ob, long oy, int ox, int B, int H, int W,
                    int K, fs_stream_t stream);
/* u=int((gx+1)/2*(W-1)), v=int((gy+1)/2*(H-1)) for n grid points.  models/models.py:644-645. */
int fs_inverse_index_maps(const float* grid, long long* u, long long* v, long n, int H, int W, fs_stream_t stream);

/* ---- convolution engine (implicit GEMM on the matrix cores) ------------------------------------ */
/* Arithmetic of the channel-aligned conv kernels (fp32 tensors and fp32 accumulation in every mode):
 *   0 "f32"    fp32 MFMA (v_mfma_f32_32x32x2_f32), one MFMA per product;
 *   1 "bf16x3" each fp32 operand split into three bf16 terms (exact to 24 significand bits), six bf16 MFMAs per product;
 *   2 "f16x2"  each operand scaled by a power of two and split into two fp16 terms (22-23 significand bits), three fp16
 *              MFMAs per product.
 * Default 2, or FS_CONV_PRECISION=f32|bf16x3|f16x2 in the environment at load time.
 * This is the library's ONE piece of process-global mutable state (like a BLAS math-mode switch): a host-side word read by the
 * conv entry points when they choose a kernel.  It is not a launch and is not ordered with streams; set it while no other
 * thread is inside a conv entry point (the Python layer sets it once at start-up, the tests between cases).  Everything
 * else the entry points need comes in through their arguments. */
int fs_set_conv_precision(int mode);
int fs_get_conv_precision(void);
/* Stream ordering without a host round trip: everything enqueued on `waiter` after this call runs after everything enqueued on
 * `signaller` before it (what torch's `waiter.wait_stream(signaller)` does: the reference gets the same ordering from the autograd
 * engine's stream guards).  Used to run a small layer's weight gradient beside the bwd-data chain. */
int fs_stream_wait(fs_stream_t waiter, fs_stream_t signaller);
/* Deterministic mode -- the reference asks for it with torch.backends.cudnn.deterministic = True (train_deform_semantic.py:680-681).
 * By default three reductions add with fp32 atomics, whose order is the workgroups' arrival order, so two runs of the same step differ
 * in the last bits of the gradients:
 *   (1) the split-K partial tiles of the bwd-weight kernels (fs_conv2d_bwd_weight, fs_linear_bwd_weight_bias: dW);
 *   (2) the bias gradient of fs_linear_bwd_weight_bias (dbias: one column sum per split and wave);
 *   (3) dK / dV of the fp32 attention backward (fs_attention_bwd), when the query range is split to fill the chip.
 * on = 1 (or FS_DETERMINISTIC=1 in the environment at load time): (1) every split writes its partial tile to its own slab of a
 * caller-provided scratch and the slabs are summed in index order; (2) likewise for the column sums (slabs in the same scratch,
 * fs_linear_bwd_weight_bias_ws_bytes); (3) the query range is not split (one workgroup per key chunk, plain stores).  Every other
 * reduction of the library is order-fixed in both modes.  Two runs of a training step are then bit-identical, whatever stream a
 * gradient was produced on (tests/test_step_invariance.py holds the three encoders' steps to that).
 * Process-global host-side word like the precision mode (same rules); costs one memset + one reduce launch per bwd-weight call. */
int fs_set_deterministic(int on);
int fs_get_deterministic(void);
/* Scratch the forward (transposed=0) / bwd-data (transposed=1) entry points can use for this shape, in bytes
 * (0 = none).  In split-precision mode 3x3 / stride 1 / pad 1 convolutions with >= 32 input channels run as a
 * halo-tiled kernel that first packs the weights, already split into bf16 terms, into this scratch; without
 * scratch (ws = NULL) they fall back to the kernel that splits weights in flight.  Host-side query, no launch. */
long fs_conv2d_workspace_bytes(int H, int W, int Cin, int Ho, int Wo, int Cout, int R, int S, int stride, int pad, int dil,
                               int transposed);
/* Which kernel family fs_conv2d_fwd (transposed=0) / fs_conv2d_bwd_data (transposed=1) select for this problem under the
 * current precision mode with ws_bytes of scratch: 0 = generic 64-bit-indexed implicit GEMM (any channel count, sources of
 * 4 GB and more), 1 = plain channel-aligned implicit GEMM, 2 = halo-tiled 3x3 stride-1 kernel, 3 = tap-class kernel,
 * 4 = 1x1 / stride-1 GEMM kernel with pre-split weights (also the forward of stride >= filter layers with 64-aligned input channels,
 * as that GEMM over gathered rows), 5 = halo-tiled 3x3 stride-1 kernel with F(2,3) minimal filtering along
 * the row (even widths; 12 instead of 18 matrix steps per pixel pair), 6 = bwd-data of a 3x3 / stride-2 / pad-1 layer with the four
 * output parities in one launch, 7 = its forward with the four input parity planes in one LDS refill per chunk, 8 = the 3x3 kernel with
 * F(4,3) minimal filtering along the row (bf16x3, widths that are multiples of 4; 18 instead of 24 matrix steps per four pixels).  The
 * aligned kernels address the source with 32-bit byte offsets, so they are chosen only below 4 GB.  Host-side predicate. */
int fs_conv2d_kernel_choice(int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int R, int S, int stride, int pad, int dil,
                            int transposed, long ws_bytes);
/* Weight packs that outlive the call.  The kernels of families 2-8 above start with a small launch that writes the layer's weights,
 * split into their 16-bit terms in consumption order, into ws; the weights only change at the optimiser step, so a caller may keep one
 * scratch per (layer, direction), fill it once per weight update -- on any stream, e.g. beside the first kernels of the next step
 * -- and run the convolutions on it (every nn.Conv2d on the path, e.g. models/hrnetv2_nodownsp.py:49-55).
 *   fs_conv2d_pack_persistent: 1 when ws of this problem is ONE pack that depends on (w, shape, precision mode) only, else 0.
 *   fs_conv2d_pack: run only that pack launch (FS_ERR_ARG when the predicate is 0; nothing is launched then).
 *   fs_conv2d_ws_mode(1): the calling thread's following conv entry points take ws as already packed for their problem and skip the
 *     pack launch, until fs_conv2d_ws_mode(0); returns the previous mode.  A problem whose kernel has no persistent pack fails with
 *     FS_ERR_ARG in mode 1 instead of running on stale scratch.  Host-side, thread-local. */
int fs_conv2d_pack_persistent(int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int R, int S, int stride, int pad, int dil,
                              int transposed, long ws_bytes);
int fs_conv2d_pack(const float* w, int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int R, int S, int stride, int pad, int dil,
                   int transposed, void* ws, long ws_bytes, const unsigned* w_amax, fs_stream_t stream);
int fs_conv2d_ws_mode(int mode);
/* Number of [Cout][2] partial-sum slabs fs_conv2d_fwd_stats writes for this shape given ws_bytes of scratch. */
int fs_conv2d_stats_slabs(int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int R, int S, int stride, int pad, int dil,
                          long ws_bytes);
/* max|w| as float bits for each of nparams weight tensors stored in one arena (tensor p = sizes[p] floats at arena + offsets[p]),
 * one launch.  A caller that keeps this up to date (train.FlatAdam does, after every step) hands &out[p] to the conv entry points
 * as w_amax and saves them the per-call reduction over the weights that the f16x2 mode needs for its weight scale. */
int fs_weight_amax_segments(const float* arena, const long* offsets, const long* sizes, int nparams, unsigned* out, fs_stream_t stream);
/* F.conv2d(x, w, bias, stride, pad, dilation=dil) [+ Dropout(drop_p) keyed by drop_key when drop_p > 0].
 * ws / ws_bytes: caller-owned scratch (see fs_conv2d_workspace_bytes), may be NULL / 0.
 * w_amax: device pointer to max|w| (float bits) of this weight tensor, or NULL (then it is computed per call when needed).
 * models/hrnetv2_nodownsp.py:49-50,54-55 and every nn.Conv2d on the path. */
int fs_conv2d_fwd(const float* x, const float* w, const float* bias, float* y, int B, int H, int W, int Cin, int Ho, int Wo,
                  int Cout, int R, int S, int stride, int pad, int dil, float drop_p, uint32_t drop_key, void* ws, long ws_bytes,
                  const unsigned* w_amax, fs_stream_t stream);
/* The forward of a linear layer that ENDS a residual branch of a transformer block (transformers' modeling_segformer.py SegformerSelfOutput /
 * SegformerMixFFN.dense2 followed by `hidden_states = drop_path(...) + hidden_states`, the network /root/reference/models/segformer.py:88-100
 * runs), with the residual add in the GEMM epilogue (round 5):   y = res + DropPath_b(Dropout(conv(x, w) + bias)).
 * Dropout: the element hash of fs_conv2d_fwd (drop_p 0 = none); DropPath: the per-sample hash of fs_residual_droppath over samples of
 * rows_per_sample consecutive output pixels (droppath_p 0 = none).  Only where the 1x1 GEMM kernel runs the layer:
 * fs_conv2d_fwd_residual_ok (host only) says so, otherwise call fs_conv2d_fwd + fs_residual_droppath. */
int fs_conv2d_fwd_residual_ok(int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int R, int S, int stride, int pad, int dil,
                              long rows_per_sample, long ws_bytes);
int fs_conv2d_fwd_residual(const float* x, const float* w, const float* bias, const float* res, float* y, int B, int H, int W, int Cin,
                           int Ho, int Wo, int Cout, int R, int S, int stride, int pad, int dil, float drop_p, uint32_t drop_key,
                           float droppath_p, uint32_t droppath_key, long rows_per_sample, void* ws, long ws_bytes, const unsigned* w_amax,
                           fs_stream_t stream);
/* Same forward conv, additionally writing per-workgroup BatchNorm partial sums of the stored output into
 * stats = [fs_conv2d_stats_slabs(...)][Cout][2] floats (needs Cin%4==0 && Cout%4==0); finalise with
 * fs_bn_finalize_slab.  Fuses the statistics pass of F.batch_norm(training=True)
 * (lib/nn/modules/batchnorm.py:58-61) into the conv. */
int fs_conv2d_fwd_stats(const float* x, const float* w, const float* bias, float* y, float* stats, int B, int H, int W, int Cin,
                        int Ho, int Wo, int Cout, int R, int S, int stride, int pad, int dil, float drop_p, uint32_t drop_key,
                        void* ws, long ws_bytes, const unsigned* w_amax, fs_stream_t stream);
/* Inference forward with the BatchNorm of eval mode folded in: z = act((conv(x, w) + bias) * scale[c] + shift[c] [+ res]),
 * scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale (lib/nn/modules/batchnorm.py:56-61 with training = False;
 * models/hrnetv2_nodownsp.py:46-62 for the residual / ReLU order), act = 0 none / 1 ReLU / 2 ReLU6.  One launch, no intermediate conv
 * output.  fs_conv2d_fwd_affine_act_ok (host only) = 1 where the kernel this shape runs on has the row epilogue, else call
 * fs_conv2d_fwd + fs_bn_eval_prepare + fs_bn_act_fwd. */
int fs_conv2d_fwd_affine_act_ok(int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int R, int S, int stride, int pad, int dil,
                                long ws_bytes);
int fs_conv2d_fwd_affine_act(const float* x, const float* w, const float* bias, const float* scale, const float* shift, const float* res,
                             float* z, int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int R, int S, int stride, int pad, int dil,
                             int act, void* ws, long ws_bytes, const unsigned* w_amax, fs_stream_t stream);
/* convolution_backward: input gradient / weight gradient (dw overwritten). */
int fs_conv2d_bwd_data(const float* dy, const float* w, float* dx, int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int R,
                       int S, int stride, int pad, int dil, void* ws, long ws_bytes, const unsigned* w_amax, fs_stream_t stream);
/* The same call where x is the output z of a conv + BatchNorm + activation layer and this convolution is its only consumer
 * (models/hrnetv2_nodownsp.py:49-56: conv1 -> bn1 -> relu -> conv2): dx is that layer's dz, and the epilogue that holds it in registers
 * also writes the layer's BatchNorm-backward partial sums (fs_bn_bwd_partial's slab) -- bn_y / bn_mask / bn_mean / bn_invstd are the
 * layer's forward record, bn_mask NULL = no activation.  add_src (nullable): a second gradient of x to be added in the same epilogue
 * -- the residual branch of a BasicBlock (models/hrnetv2_nodownsp.py:59-62): add_src = the block's last BatchNorm's dz, add_mask its
 * activation bits (1 byte per 4 channels, NULL = unmasked) -- so autograd's add at the block input disappears as well (bn_y may be NULL
 * when only the addend is wanted).
 * fs_conv2d_bwd_data_bnsum_slabs (host only) gives the slab's row count, or 0 when the kernel this shape runs on cannot form the sums
 * (then call fs_conv2d_bwd_data + fs_bn_bwd_partial).  Kernels that can: the 3x3 stride-1 row-transform family (round 3), and since
 * round 5 the 1x1 GEMM kernel (hrnetv2_nodownsp.py:96-103: conv2 -> bn2 -> relu -> conv3 of a Bottleneck) and the one-launch 3x3 /
 * stride-2 kernel (hrnetv2_nodownsp.py:160-176: the first convolution of a two-step fuse down-path). */
int fs_conv2d_bwd_data_bnsum_slabs(int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int R, int S, int stride, int pad, int dil,
                                   long ws_bytes);
int fs_conv2d_bwd_data_bnsum(const float* dy, const float* w, float* dx, int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int R,
                             int S, int stride, int pad, int dil, void* ws, long ws_bytes, const unsigned* w_amax, const float* bn_y,
                             const unsigned char* bn_mask, const float* bn_mean, const float* bn_invstd, float* slab, const float* add_src,
                             const unsigned char* add_mask, fs_stream_t stream);
/* nn.Linear backward w.r.t. its parameters in one launch (the ATen addmm / sum backward behind transformers' modeling_segformer linears,
 * call sites models/segformer.py:9-11,33-37): dw[Cin][Cout] = x^T dy over `rows` rows, dbias[Cout] = column sums of dy.  Exists in the
 * bf16x3 mode for Cin, Cout multiples of 4 and >= 16 (fs_linear_bwd_weight_bias_ok == 1); otherwise FS_ERR_ARG -- callers then use
 * fs_conv2d_bwd_weight + fs_colsum.  accumulate_w / accumulate_b as `accumulate` below. */
int fs_linear_bwd_weight_bias_ok(long rows, int Cin, int Cout);
long fs_linear_bwd_weight_bias_ws_bytes(int Cin, int Cout);
int fs_linear_bwd_weight_bias(const float* x, const float* dy, float* dw, float* dbias, long rows, int Cin, int Cout, int accumulate_w,
                              int accumulate_b, void* ws, long ws_bytes, fs_stream_t stream);
/* accumulate = 0: dw is overwritten; 1: the gradient is ADDED to dw (torch's .grad accumulation; saves the memset when the caller
 * keeps a zeroed gradient arena).  ws / ws_bytes: scratch for the per-split partial tiles of deterministic mode --
 * fs_conv2d_bwd_weight_ws_bytes (0 outside that mode; ws may then be NULL).  In deterministic mode a missing or short scratch is
 * FS_ERR_ARG: the call never falls back to the atomics silently. */
long fs_conv2d_bwd_weight_ws_bytes(int Cin, int Cout, int R, int S, int stride, int pad, int dil);
/* What fs_conv2d_bwd_weight does with this problem under the current precision and deterministic modes and ws_bytes of scratch
 * (ws_bytes > 0 stands for "scratch given"; accumulate = 0).  Returns 1 when the call would be accepted, else 0.  out[6] receives
 *   out[0] route: 0 = generic kernel, 1 = generic kernel with float4 loads (channel counts multiples of 4), 2 / 3 = fp32 3x3 kernel with 3 / 9
 *          taps per workgroup, 4 = split-precision 3x3 stride-1 class kernel, 5 = transform-domain 3x3 kernel, 6 = linear-layer GEMM
 *          (1x1 / stride 1), 7 = one GEMM per tap over gathered rows in one launch, 8 = strided 3x3 over parity planes in one launch,
 *          9 = one launch per tap class;
 *   out[1] accumulation over the pixel splits: 0 = atomics into dw after a memset of it, 1 = atomics into an accumulating dw (reported by
 *          calls with accumulate != 0 only), 2 = zeroed slabs in ws + ordered sum, 3 = slabs written without a memset + ordered sum;
 *   out[2] convolution kernel launches (memsets and the sum not counted), out[3] their workgroups together, out[4] threads per workgroup,
 *   out[5] slab rows of R*S*Cin*Cout floats the launches write in ws (0 with atomics).
 * All zero for an invalid shape.  Host-side, no launch. */
int fs_conv2d_bwd_weight_plan(int B, int H, int W, int Cin, int Ho, int Wo, int Cout, int R, int S, int stride, int pad, int dil, long ws_bytes,
                              int* out);
int fs_conv2d_bwd_weight(const float* x, const float* dy, float* dw, int B, int H, int W, int Cin, int Ho, int Wo, int Cout,
                         int R, int S, int stride, int pad, int dil, int accumulate, void* ws, long ws_bytes, fs_stream_t stream);

/* ---- BatchNorm / activation / residual ------------------------------------------------------ */
/* F.batch_norm(training=True) statistics over M rows; running stats updated in place (nullable).
 * lib/nn/modules/batchnorm.py:56-61.  sums = fs_bn_stats_scratch_doubles(M, C) doubles of scratch (per-row-block records, added in
 * block order). */
long fs_bn_stats_scratch_doubles(long M, int C);
int fs_bn_stats(const float* y, long M, int C, float momentum, float eps, float* running_mean, float* running_var, float* mean,
                float* invstd, double* sums, fs_stream_t stream);
int fs_bn_finalize_slab(const float* slab, int nwg, long M, int C, float momentum, float eps, float* running_mean,
                        float* running_var, float* mean, float* invstd, fs_stream_t stream);
int fs_bn_eval_prepare(const float* running_mean, const float* running_var, int C, float eps, float* mean, float* invstd,
                       fs_stream_t stream);
/* the same statistics as the two per-channel coefficients fs_conv2d_fwd_affine_act takes: scale = gamma / sqrt(running_var + eps),
 * shift = beta - running_mean * scale */
int fs_bn_eval_affine(const float* running_mean, const float* running_var, const float* gamma, const float* beta, int C, float eps,
                      float* scale, float* shift, fs_stream_t stream);
/* out = act((y-mean)*invstd*gamma + beta [+ res]).  mask (nullable, M*C/4 bytes): bit j of byte e/4 = act'(out[e+j]) != 0, so the
 * backward passes read one byte instead of four floats of `out`.  models/hrnetv2_nodownsp.py:51-52,56-62. */
int fs_bn_act_fwd(const float* y, const float* mean, const float* invstd, const float* gamma, const float* beta, const float* res,
                  float* out, unsigned char* mask, long M, int C, int act, fs_stream_t stream);
/* Backward of the above (F.batch_norm backward + activation + dropout mask of the conv output; models/hrnetv2_nodownsp.py:46-62,
 * lib/nn/modules/batchnorm.py:56-61) in three stages; the activation derivative comes from `mask` when given, else from z (= out):
 *   fs_bn_bwd_partial : column sums sum(g), sum(g * xhat) of g = dz * act'(z) per block of rows -> slab[fs_bn_bwd_slabs(M, C)][C][2].
 *                       Skipped when the kernel that produced dz wrote the slab itself (fs_add_n_bnsum).
 *   fs_bn_bwd_finalize: slab -> dgamma, dbeta (accumulate_affine != 0: ADDED to gradient-arena targets, else overwritten) and the
 *                       per-channel coefficients coef[4][C] of the apply pass (training = 0: running statistics, no mean terms).
 *   fs_bn_bwd_apply   : dy = gradient w.r.t. the (dropped-out) conv output, dres (nullable) = gradient w.r.t. the residual input. */
int fs_bn_bwd_slabs(long M, int C);      /* host only */
int fs_bn_bwd_partial(const float* dz, const float* z, const unsigned char* mask, const float* y, const float* mean, const float* invstd,
                      long M, int C, int act, float* slab, fs_stream_t stream);
int fs_bn_bwd_finalize(const float* slab, int nslab, const float* gamma, const float* mean, const float* invstd, long M, int C,
                       int training, float* coef, float* dgamma, float* dbeta, int accumulate_affine, fs_stream_t stream);
int fs_bn_bwd_apply(const float* dz, const float* z, const unsigned char* mask, const float* y, const float* coef, long M, int C, int act,
                    float drop_p, uint32_t drop_key, float* dy, float* dres, fs_stream_t stream);

/* ---- HRNet multi-resolution fuse / concat ------------------------------------------------------ */
/* out = [relu](sum_t up(terms[t])), terms at (th[t],tw[t]) bilinearly up-sampled (align_corners=False).
 * models/hrnetv2_nodownsp.py:235-251.  terms/th/tw are HOST arrays of length nterms (<= 4). */
int fs_hr_fuse_fwd(const float* const* terms, const int* th, const int* tw, int nterms, float* out, int B, int Ho, int Wo, int C,
                   int relu, fs_stream_t stream);
int fs_relu_bwd(const float* dout, const float* out, float* g, long n, fs_stream_t stream);
/* out = a + b [+ c [+ d]] over n floats (n % 4 == 0; c, d may be NULL; out may alias a): the sum of the gradients that reach a tensor
 * with several consumers -- the block input of models/hrnetv2_nodownsp.py:46-64 (conv path + residual), the branch outputs every
 * fuse row reads (:228-252) -- which the autograd engine would otherwise form with ATen's binary add, one launch per extra consumer. */
int fs_add_n(const float* a, const float* b, const float* c, const float* d, float* out, long n, fs_stream_t stream);
/* The same sum where `out` is the gradient of a conv + BatchNorm + activation layer's output (autograd's add at the BasicBlock
 * output, models/hrnetv2_nodownsp.py:59-62): also writes that layer's BatchNorm-backward partial sums (fs_bn_bwd_partial's slab),
 * so the layer's own reduction pass is skipped.  mask / y / mean / invstd: the layer's forward record; M rows of C channels. */
int fs_add_n_bnsum(const float* a, const float* b, const float* c, const float* d, float* out, const unsigned char* mask, const float* y,
                   const float* mean, const float* invstd, long M, int C, int act, float* slab, fs_stream_t stream);
/* dst[..., coff:coff+C] = up(src); models/hrnetv2_nodownsp.py:434-442 (interpolate + cat). */
int fs_upsample_slice_fwd(const float* src, int B, int th, int tw, int C, float* dst, int Ho, int Wo, int Cdst, int coff,
                          fs_stream_t stream);
int fs_upsample_slice_bwd(const float* g, int B, int Ho, int Wo, int Cg, int coff, float* dsrc, int th, int tw, int C,
                          fs_stream_t stream);
/* Round 5: the two producers of an HRNet fuse row's gradients also form the BatchNorm-backward column sums of the layers that receive them
 * (models/hrnetv2_nodownsp.py:179-252: the last ConvBn of every fuse path has no activation, so its output gradient IS the fuse gradient):
 *   fs_relu_bwd_bnsum: g = dout * (out > 0) over (M rows, C channels, C <= 1024) and, for nterm <= 3 layers k with conv output y[k] and batch
 *     statistics mean[k] / invstd[k], slab[k][fs_bn_bwd_slabs(M, C)][C][2] = per-row-block (sum g, sum g * xhat_k) -- the input of fs_bn_bwd_finalize.
 *     y / mean / invstd / slab are HOST arrays of nterm device pointers.
 *   fs_upsample_slice_bwd_bnsum: fs_upsample_slice_bwd (even up-sampling factors) plus slab[fs_bn_bwd_slabs(B*th*tw, C)][C][2] of the layer
 *     whose output gradient dsrc is. */
int fs_relu_bwd_bnsum(const float* dout, const float* out, float* g, long M, int C, int nterm, const float* const* y, const float* const* mean,
                      const float* const* invstd, float* const* slab, fs_stream_t stream);
int fs_upsample_slice_bwd_bnsum(const float* g, int B, int Ho, int Wo, int Cg, int coff, float* dsrc, int th, int tw, int C, const float* y,
                                const float* mean, const float* invstd, float* slab, fs_stream_t stream);
/* column sums of M rows of C floats (bias gradients); accumulate != 0: ADDED to out (a gradient-arena target), else overwritten.
 * scratch = fs_colsum_scratch_floats(M, C) floats (per-row-block partial sums, added in block order). */
long fs_colsum_scratch_floats(long M, int C);
int fs_colsum(const float* x, long M, int C, float* out, int accumulate, float* scratch, fs_stream_t stream);
/* nn.MaxPool2d(k, stride, pad) on NHWC; arg = flat input pixel index of the maximum (int32), used by the backward.
 * torchvision ResNet stem behind models/deeplab.py:15. */
int fs_maxpool_fwd(const float* x, float* out, int* arg, int B, int H, int W, int C, int Ho, int Wo, int k, int stride, int pad,
                   fs_stream_t stream);
int fs_maxpool_bwd(const float* dout, const int* arg, float* dx, int B, int H, int W, int C, int Ho, int Wo, int k, int stride,
                   int pad, fs_stream_t stream);
/* nn.Dropout(p) as a stand-alone pass (same call for forward and backward); hash mask keyed by drop_key. */
int fs_dropout(const float* x, float* out, long n, float drop_p, uint32_t drop_key, fs_stream_t stream);
/* AvgPool2d((10,10)) on a 10x10 map.  models/model_utils.py:254,272. */
int fs_avgpool_fwd(const float* x, int B, int HW, int C, float* out, fs_stream_t stream);
int fs_avgpool_bwd(const float* dout, int B, int HW, int C, float* dx, fs_stream_t stream);

/* ---- C1 head tail + losses --------------------------------------------------------------------- */
/* m = sigmoid(w . x + bias) - 0.5 per pixel.  models/model_utils.py:293-298. */
int fs_mask_head_fwd(const float* x, const float* w, const float* bias, float* m, long npix, int C, fs_stream_t stream);
/* scratch = fs_mask_head_bwd_scratch_floats(npix, C) floats (per-workgroup partial sums of dw and db, added in workgroup order) */
long fs_mask_head_bwd_scratch_floats(long npix, int C);
int fs_mask_head_bwd(const float* dm, const float* m, const float* x, const float* w, float* dx, float* dw, float* db, long npix,
                     int C, float* scratch, fs_stream_t stream);
/* pred (B,K,HW) NCHW: pred[:, :K-1] = cls, pred[:, K-1] = cls[K-1]*m.  models/model_utils.py:300-306. */
int fs_pred_assemble_fwd(const float* cls, const float* m, float* pred, int B, int K, int HW, fs_stream_t stream);
int fs_pred_assemble_bwd(const float* dpred, const float* cls, const float* m, float* dcls, float* dm, int B, int K, int HW,
                         fs_stream_t stream);
/* out[7] = {dice+focal, focal, dice, acc, acc_bin_fg, acc_cls_fbg, acc_bin_fbg}; models/models.py:87-120,378-474,1057-1078.
 * accum = B * ceil(HW/1024) * (3K+7) doubles of scratch (one record per workgroup, no initialisation needed),
 * coef = 2K floats kept for the backward. */
int fs_seg_loss_fwd(const float* pred, const long long* gt, int B, int K, int HW, float gamma, float eps, double* accum,
                    float* out, float* coef, fs_stream_t stream);
int fs_seg_loss_bwd(const float* pred, const long long* gt, const float* coef, const float* gout, float* dpred, int B, int K,
                    int HW, float gamma, fs_stream_t stream);

/* ---- SegFormer (Mix-Transformer) encoder pieces; tokens are NHWC rows (B, N=H*W, C) ------------------------
 * third-party transformers==4.46.2 modeling_segformer behind models/segformer.py:9-60,87-105 */
/* nn.LayerNorm(C, eps) over the last dim of M rows; mean/rstd (M floats each) kept for the backward. */
int fs_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, long M, int C,
                     float eps, fs_stream_t stream);
/* accumulate != 0: dgamma / dbeta are ADDED to (gradient-arena targets), else overwritten.  scratch =
 * fs_layernorm_bwd_scratch_floats(M, C) floats (per-workgroup records of the two column sums, added in workgroup order). */
long fs_layernorm_bwd_scratch_floats(long M, int C);
int fs_layernorm_bwd(const float* g, const float* x, const float* gamma, const float* mean, const float* rstd, float* dx,
                     float* dgamma, float* dbeta, long M, int C, int accumulate, float* scratch, fs_stream_t stream);
/* The same pass with a second gradient of x added to dx (round 5): x of a pre-norm block feeds the LayerNorm and the residual add
 * (transformers' modeling_segformer.py SegformerLayer.forward, used by /root/reference/models/segformer.py:88-100), so the residual's gradient
 * arrives beside the LayerNorm's; adding it here replaces the autograd engine's add pass (104 per configs[3] step).  addend NULL = fs_layernorm_bwd. */
int fs_layernorm_bwd_add(const float* g, const float* x, const float* gamma, const float* mean, const float* rstd, const float* addend,
                         float* dx, float* dgamma, float* dbeta, long M, int C, int accumulate, float* scratch, fs_stream_t stream);
/* exact (erf) GELU. */
int fs_gelu_fwd(const float* x, float* y, long n, fs_stream_t stream);
int fs_gelu_bwd(const float* g, const float* x, float* dx, long n, fs_stream_t stream);
/* nn.GELU followed by nn.Dropout(p) (SegformerMixFFN: intermediate_act_fn, dropout; transformers 4.46.2, models/segformer.py:2,88-100) in
 * one pass, and the backward of the pair in one pass: the mask of fs_dropout with the same key on the same element index.  n < 2^32. */
int fs_gelu_dropout_fwd(const float* x, float* y, long n, float drop_p, uint32_t key, fs_stream_t stream);
int fs_gelu_dropout_bwd(const float* g, const float* x, float* dx, long n, float drop_p, uint32_t key, fs_stream_t stream);
/* depthwise Conv2d(C, C, 3, 1, 1, groups=C) on NHWC, weight (C,1,3,3); flip=1 gives the input gradient. */
int fs_dwconv3_fwd(const float* x, const float* w, const float* bias, float* y, int B, int H, int W, int C, int flip,
                   fs_stream_t stream);
/* weight gradient: ws = fs_dwconv3_wgrad_lanes(B, H, W, C) * 9 * C floats of scratch (per-thread partial sums, added up by a second
 * launch: no atomics, no memset); accumulate != 0: dw is ADDED to, else overwritten. */
int fs_dwconv3_wgrad_lanes(int B, int H, int W, int C);      /* host only */
int fs_dwconv3_bwd_weight(const float* x, const float* dy, float* dw, float* ws, int B, int H, int W, int C, int accumulate,
                          fs_stream_t stream);
/* ... with the bias gradient db[C] = column sums of dy formed by the same two launches (the kernel reads every dy element exactly once
 * already; a separate column-sum pass re-read 131 MB per Mix-FFN block of configs[3]): ws = lanes * 10 * C floats. */
int fs_dwconv3_bwd_weight_bias(const float* x, const float* dy, float* dw, float* db, float* ws, int B, int H, int W, int C,
                               int accumulate_w, int accumulate_b, fs_stream_t stream);
/* out = x + DropPath_p(y) (per-sample keep, hash keyed); x NULL -> out = scaled y (the backward of the y branch). */
int fs_residual_droppath(const float* x, const float* y, float* out, long n, long per_sample, float drop_p, uint32_t key,
                         fs_stream_t stream);
/* ... and that form's gradient with respect to the layer's output in one pass: dz = Dropout-mask(DropPath-scale_b * g), the two masks in
 * the order fs_residual_droppath (x = NULL) followed by fs_dropout apply them.  n < 2^32, n and per_sample multiples of 4. */
int fs_droppath_dropout_bwd(const float* g, float* dz, long n, long per_sample, float droppath_p, uint32_t droppath_key, float drop_p,
                            uint32_t drop_key, fs_stream_t stream);
/* A convolution whose filter has more taps than the aligned kernels take (SegFormer's 7x7 patch embedding on 3 channels and 8x8 stride-8
 * sequence-reduction conv: transformers 4.46.2 SegformerOverlapPatchEmbeddings / SegformerEfficientSelfAttention.sr, models/segformer.py:
 * 9-11,33-37) as patch rows: col[B*Ho*Wo][Kp], element (r, s, c) of the k x k patch in the RSCK weight's row order, zeros outside the image
 * and in the padding columns (Kp % 4 == 0) -- the layer is then one linear layer.  fs_fold is the adjoint (dx overwritten). */
int fs_unfold(const float* x, float* col, int B, int H, int W, int C, int k, int stride, int pad, int Ho, int Wo, int Kp, fs_stream_t stream);
int fs_fold(const float* col, float* dx, int B, int H, int W, int C, int k, int stride, int pad, int Ho, int Wo, int Kp, fs_stream_t stream);
/* softmax(q k^T * scale) (dropout p) v per head on the matrix cores (v_mfma_f32_32x32x2_f32: exact fp32 products, fp32
 * accumulate); head_dim 64, any number Nk of sequence-reduced key/value tokens (streamed in chunks of 64, online softmax);
 * q/o (B,N,heads*64), k/v (B,Nk,heads*64); lse = B*heads*N floats (log-sum-exp per query row, kept for the backward).
 * Replaces SegformerEfficientSelfAttention's matmul-softmax-dropout-matmul (transformers 4.46.2, models/segformer.py:2,88-100). */
int fs_attention_fwd(const float* q, const float* k, const float* v, float* o, float* lse, int B, int N, int Nk, int heads,
                     float scale, float drop_p, uint32_t key, fs_stream_t stream);
/* The same forward in split precision (bf16x3: q*scale, k, v and the probabilities as three bf16 planes = 24-bit operands, six
 * v_mfma_f32_32x32x16_bf16 per product, fp32 accumulation and softmax) -- the arithmetic of the conv engine's headline mode, 3/8 of the
 * matrix-pipe time of the exact kernel.  ws = fs_attention_split_ws_bytes(B, Nk, heads) bytes of scratch (K / V^T planes, written by a
 * pre-pass inside the call).  Same dropout hash and element index as fs_attention_fwd.  csrc/attention_split.hip. */
long fs_attention_split_ws_bytes(int B, int Nk, int heads);
/* mask (nullable) = fs_attention_mask_words(B, N, Nk, heads) words: with drop_p > 0 the forward leaves the keep decisions there, one bit per
 * (query, key) -- row (b*heads + head)*N + q, word key >> 5, bit key & 31 -- and the split backward reads them instead of hashing again. */
long fs_attention_mask_words(int B, int N, int Nk, int heads);
int fs_attention_fwd_split(const float* q, const float* k, const float* v, float* o, float* lse, unsigned* mask, void* ws, long ws_bytes,
                           int B, int N, int Nk, int heads, float scale, float drop_p, uint32_t key, fs_stream_t stream);
/* Backward of the above: dq, dk, dv overwritten.  o = the forward's output, go = its gradient, scratch = B*heads*N floats. */
int fs_attention_bwd(const float* q, const float* k, const float* v, const float* o, const float* go, const float* lse, float* dq,
                     float* dk, float* dv, float* scratch, int B, int N, int Nk, int heads, float scale, float drop_p, uint32_t key,
                     fs_stream_t stream);
/* The backward in split precision (bf16x3): dQ with the query on the MFMA lane (transposed score tile, dS fed to the K^T product from
 * registers), dK and dV with the key on the lane (P~ / dS fed to the dO^T / Q^T products from registers, the query-slice images read by rows
 * and transposed), no LDS round trip for P or dS.  ws = fs_attention_bwd_split_ws_bytes(B, Nk, heads) bytes of scratch (the dQ kernel's
 * K / V / K^T planes); mask = the forward's keep words or NULL (the kernels then hash again).  fs_attention_bwd_dq_split / _dkv_split are
 * the two parts alone (D = rowsum(dO * O), B*heads*N floats). */
long fs_attention_bwd_split_ws_bytes(int B, int Nk, int heads);
int fs_attention_bwd_dq_split(const float* q, const float* k, const float* v, const float* go, const float* lse, const float* D,
                              const unsigned* mask, float* dq, void* ws, long ws_bytes, int B, int N, int Nk, int heads, float scale,
                              float drop_p, uint32_t key, fs_stream_t stream);
/* parts (nullable): 2 * 8 * B * Nk * heads * 64 floats for the partial dK / dV of up to 8 splits of the query range (summed by a small
 * kernel; without it the range is not split).  fs_attention_bwd_split carves it from its ws at fs_attention_bwd_split_parts_offset. */
long fs_attention_bwd_split_parts_offset(int B, int Nk, int heads);
int fs_attention_bwd_dkv_split(const float* q, const float* k, const float* v, const float* go, const float* lse, const float* D,
                               const unsigned* mask, float* dk, float* dv, float* parts, int B, int N, int Nk, int heads, float scale,
                               float drop_p, uint32_t key, fs_stream_t stream);
int fs_attention_bwd_split(const float* q, const float* k, const float* v, const float* o, const float* go, const float* lse,
                           const unsigned* mask, float* dq, float* dk, float* dv, float* scratch, void* ws, long ws_bytes, int B, int N,
                           int Nk, int heads, float scale, float drop_p, uint32_t key, fs_stream_t stream);

/* ---- optimiser ------------------------------------------------------------------------------- */
/* torch.optim.Adam(weight_decay) step over a flat fp32 arena of n (multiple of 4) elements; step >= 1;
 * grad_scale multiplies the gradient first (1/world_size).  train_deform_semantic.py:115-123,271-288. */
int fs_adam_step(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
                 float weight_decay, int step, float grad_scale, fs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
