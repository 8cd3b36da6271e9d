/*
 * ttnet.h -- C ABI of the MI355X-native TTNet inference path (libttnet.so).
 *
 * This is the drop-in boundary for ONE path of Anonymousijcai2024ttnet/scale_imagenet: the
 * eval-mode forward() of the TTNet ImageNet classifiers.  The reference has no FFI (it is
 * 100 % PyTorch), so each entry point below names the reference interface it replaces
 * (file:line under the upstream repository) and INTEGRATION.md shows the ctypes stub a
 * maintainer adds to the reference's nn.Module to call it.
 *
 * Conventions
 *   - plain C types only; device pointers are raw HIP device addresses; `stream` is a
 *     hipStream_t passed as void* (NULL = the null stream).
 *   - every function returns 0 on success or a negative ttnet_status; the message for the
 *     last failure on the calling thread is ttnet_last_error().
 *   - a plan is bound to one device; calls on one plan are serialised by the caller;
 *     different plans may run concurrently on different streams.
 *   - device memory is allocated only inside ttnet_plan_create / _finalize / _set_lanes
 *     (weights, truth tables, one activation workspace for `max_batch` images per lane);
 *     ttnet_forward never synchronises.  It instantiates a hipGraph of its own the third time
 *     a batch size is seen (and replays it afterwards); when the caller's stream is itself
 *     capturing, it records plain launches into the caller's graph instead.
 *   - there is no CPU fallback: without a HIP device every compute entry point fails.
 *
 * Packed activation layouts (all little-endian, LSB first)
 *   rows  ("RP"): uint64 [N][C][H]      bit x of word (n,c,y) is pixel (y,x); W <= 60
 *   chans ("CP"): uint16 [N][C/16][H][W] bit k of word (n,q,y,x) is channel 16q+k
 */
#ifndef TTNET_H
#define TTNET_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ttnet_plan ttnet_plan;
typedef struct ttnet_comm ttnet_comm;

typedef enum ttnet_status {
  TTNET_OK = 0,
  TTNET_E_INVALID = -1,      /* bad argument (NULL, shape, unknown key, batch > max_batch) */
  TTNET_E_STATE = -2,        /* call out of order (forward before finalize, missing tensor) */
  TTNET_E_HIP = -3,          /* a HIP runtime call failed; message carries hipGetErrorString */
  TTNET_E_UNSUPPORTED = -4,  /* geometry this build has no kernel for */
  TTNET_E_NOMEM = -5,
  TTNET_E_RANGE = -6         /* an earlier forward met a value outside the fp16 x 2 operand split (see ttnet_forward) */
} ttnet_status;

typedef enum ttnet_dtype { TTNET_F32 = 0, TTNET_I64 = 1, TTNET_U8 = 2, TTNET_U16 = 3, TTNET_U64 = 4 } ttnet_dtype;

typedef enum ttnet_variant {
  TTNET_SMALL = 0,   /* models/TT_general_imagenet_v2_small.py:151  TT_vf_19lv3_imgnet_small  */
  TTNET_XSMALL = 1,  /* models/TT_general_imagenet_v2_xsmall.py:151 TT_vf_19lv3_imgnet_xsmall */
  TTNET_FULL = 2,    /* models/TT_general_imagenet_v2.py:139        TT_vf_19lv3_imgnet        */
  TTNET_VALEXNET = 3 /* models/TT_FHE_XSMALL_vAlexnet.py:585        TT_FHE_XSMALL_vAlexnet (CIFAR 32x32;
                        nfilter / tfilter / layers are ignored, as the reference's constructor ignores them) */
} ttnet_variant;

/* The constructor arguments of the reference model (args.nfilter / tfilter / layers,
 * models/TT_general_imagenet_v2_small.py:154-181; main.py:47-50) plus what the reference
 * discovers with a dry run on torch.rand(1,3,224,224) (:199-207): the input size.
 *
 * Which (variant, p = nfilter * tfilter, layers) the reference constructs and this library builds
 * (everything else: ttnet_plan_create returns TTNET_E_UNSUPPORTED with the reason in ttnet_last_error):
 *   TTNET_SMALL    reference: any p for which nn.Conv2d accepts groups = int(C / 16) for C = p, 2p, 4p .. and 4C
 *                  (:28-76; e.g. every multiple of 16, but also p = 40 with a fan-in of 20), layers 0..4.
 *                  built: p in {16, 32, .., 128} (fan-in 16: the truth-table kernels; the stem kernel holds one, two or
 *                  four 32-channel M-tiles), layers 0..2; layers 3 / 4 (stride-1 blocks) at p = 64.  Not built: p > 128,
 *                  p % 16 != 0.
 *   TTNET_XSMALL   reference: any p with p % 4 == 0 ..., layers 0..4.  built: p in {16, 32, .., 128} (its depthwise tables are
 *                  striped by 16 channels), layers 0..2 (the stride-1 first blocks of layers 3 / 4 exist for TTNET_SMALL only).
 *   TTNET_FULL     reference: p = 60 and the other p for which int(4C / 30) divides 4C (p = 64 does NOT construct,
 *                  SURVEY 2 #2), layers 0..3 (its --layers 2 falls through the reference's own branch-padding rules at the 9 x 9
 *                  input of the fourth block, TT_general_imagenet_v2.py:98-128).  built: those p <= 64, layers 0..1.
 *   TTNET_VALEXNET fixed geometry.
 * image_h = image_w = 224 (32 for TTNET_VALEXNET): the reference's branch-padding rules are keyed by the widths that
 * 224 x 224 produces (:98-139); other input sizes fall through them in the reference and are refused here. */
typedef struct ttnet_net_desc {
  int32_t variant;     /* ttnet_variant */
  int32_t nfilter;     /* main.py:47, default 8 */
  int32_t tfilter;     /* main.py:48, default 8 */
  int32_t layers;      /* main.py:50, default 1 */
  int32_t image_h;     /* 224 */
  int32_t image_w;     /* 224 */
  int32_t max_batch;   /* workspace is sized for this many images per forward */
  int32_t reserved;
} ttnet_net_desc;

/* Replaces TT_vf_19lv3_imgnet_small.__init__ / make_small_network
 * (models/TT_general_imagenet_v2_small.py:154-203): fixes the geometry, allocates device
 * storage for the 174 state tensors and the activation workspace. */
int ttnet_plan_create(const ttnet_net_desc *desc, int device, ttnet_plan **out);

/* Replaces nn.Module.load_state_dict (main.py:220-222): hands the plan one state_dict
 * entry under its reference key, e.g. "features.4.Block_conv1.conv1.weight".  A leading
 * "module." (DataParallel / DDP checkpoints, main.py:181-192) is accepted and stripped.
 * `ptr` may be a host or a device pointer (on_device != 0); the bytes are copied.
 * num_batches_tracked and grad_scale entries are accepted and ignored (eval mode never
 * reads them).  Unknown keys and shape / dtype mismatches are TTNET_E_INVALID, as strict
 * load_state_dict would raise. */
int ttnet_plan_set_tensor(ttnet_plan *plan, const char *key, const void *ptr,
                          const int64_t *shape, int ndim, int dtype, int on_device);

/* Derived state, rebuilt after the tensors change: folds every BatchNorm, enumerates every
 * binarised Block_TT into its truth table on the GPU (float64, exact erf; the enumeration
 * convention of Block_TT.get_TT_block_all_filter, models/TT_FHE_SMALL.py:322-342), builds
 * the float table of the last block, permutes lin1 to the feature order of the device
 * kernels.  Fails with TTNET_E_STATE if a required tensor was never set. */
int ttnet_plan_finalize(ttnet_plan *plan, void *stream);

/* Replaces SeqBinModelHelper.forward (models/model_utils/netbin.py:703-708), i.e.
 * `outputs = model(inputs)` at main.py:261 in eval mode under no_grad.
 *   x_dev      float32 [n,3,image_h,image_w] NCHW, contiguous, on the plan's device
 *   logits_dev float32 [n,n_classes]  (1000; 10 for TTNET_VALEXNET)
 * Asynchronous on `stream`.  From the third call with the same n the launches are replayed from a
 * hipGraph captured on a private stream (the input / logits pointers are patched per call);
 * TTNET_NO_GRAPH=1 in the environment keeps plain launches.  Results are identical either way.
 * Setting a tensor, a table, the input normalisation or finalizing drops every captured graph (they are re-captured).
 * Range.  The float stages run on the 16-bit matrix cores with every float32 operand carried as two
 * fp16 terms after a power-of-two prescale (x16 for activations): inputs, pooled features and
 * classifier activations must satisfy |v| < 4094 (the reference's float32 path has no such limit;
 * normalised ImageNet inputs span [-2.2, 2.7]).  A value outside the range, or a NaN, raises a sticky
 * flag from inside the kernel; since the forward is asynchronous, it is the NEXT call on the plan
 * (forward, read_stage) that fails with TTNET_E_RANGE, and keeps failing until
 * ttnet_plan_query("range_overflow") has read and cleared the flag.
 * Alignment.  x_dev must be 16-byte aligned (the stem reads it with 16-byte buffer loads; any tensor
 * torch allocates is): TTNET_E_INVALID otherwise.  The uint8 input of ttnet_forward_u8 needs 4 bytes. */
int ttnet_forward(ttnet_plan *plan, const float *x_dev, int64_t n, float *logits_dev, void *stream);

/* Batches in flight.  A plan starts with one lane = one set of activation buffers; lanes share
 * the weights and truth tables.  ttnet_plan_set_lanes grows the plan to `lanes` sets (1..16),
 * and ttnet_forward_lane runs a forward on one of them: forwards on different lanes may be in
 * flight together on different streams (the ramp and tail of one batch's kernels are filled by
 * another's; this is how the eval loop of main.py:255-275 is pipelined, evaluate.py).  Calls on
 * one plan are still issued from one thread at a time; a lane must not be reused before the
 * forward issued on it has finished or been ordered before the new one by its stream.
 * ttnet_forward is lane 0.  ttnet_read_stage, ttnet_forward_from_stem_bits and the
 * "full_listed_*" queries of ttnet_plan_query work on the lane used last: the lane of the latest
 * ttnet_forward / _lane / _u8 call that passed its argument checks (lane 0 before any). */
int ttnet_plan_set_lanes(ttnet_plan *plan, int lanes);
int ttnet_forward_lane(ttnet_plan *plan, int lane, const float *x_dev, int64_t n, float *logits_dev, void *stream);

/* SURVEY 8(f) N1 -- the tail of the input pipeline fused into the stem.  x is the decoder's
 * uint8 image, HWC: uint8 [n][image_h][image_w][3]; the library applies ToTensor (/255) and
 * Normalize(mean, std) (utils/preprocess.py:104-108; the ImageNet constants by default,
 * ttnet_plan_set_input_norm replaces them) in front of the stem's average pool.  Same result as
 * ttnet_forward on the normalised float32 tensor up to stem near ties (the stem works on the exact integer byte
 * sums, with the normalisation folded into its weights: two matrix products per output instead of the three the
 * float32 input needs).
 * TTNET_VALEXNET takes the CIFAR bytes the same way: uint8 [n][32][32][3], 4-byte aligned, any lane.  Its defaults are
 * the reference's CIFAR constants (cifar_transform, utils/preprocess.py:82-87: mean 0.4914, 0.4822, 0.4465, std 0.2023,
 * 0.1994, 0.2010).  Its stem kernel accumulates centred bytes b - round(255 mean_c), exact in float32, on weights scaled
 * by 1 / (255 std_c); the remainder of the normalisation joins the bias in one constant per border class of the
 * convolution output (interior, top row, left column, corner), because the zero padding is zero in normalised space
 * and not byte 0.  Same bits as ttnet_forward on the normalised float32 tensor up to stem near ties.
 * ttnet_plan_set_input_norm rebuilds the folded operands (at once on a finalized plan, otherwise at finalize) and
 * drops every captured graph, as setting a tensor does; std must be positive (TTNET_E_INVALID). */
int ttnet_plan_set_input_norm(ttnet_plan *plan, const float *mean3, const float *std3);
int ttnet_forward_u8(ttnet_plan *plan, int lane, const uint8_t *x_nhwc_dev, int64_t n, float *logits_dev, void *stream);

/* SURVEY 8(f) N1, the part in front of ttnet_forward_u8: transforms.Resize(resize) followed by
 * transforms.CenterCrop(crop) of the eval transform (utils/preprocess.py:104-105; 256 / 224 there) on a batch of
 * n decoded images of one size, uint8 HWC [n][h][w][3] -> uint8 [n][crop][crop][3], both on the device.
 * Resize is torchvision's resize of a PIL image, i.e. Pillow's bilinear resampling with antialiasing in
 * 8-bit fixed point (horizontal pass, then vertical); the output size and crop offsets follow
 * torchvision.transforms.functional (shorter side -> resize, longer side int(resize * long / short);
 * offsets int(round((size - crop) / 2.0))).  Not bound to a plan.  Asynchronous on `stream` (one kernel; the first call with a
 * geometry uploads its coefficient tables synchronously and keeps them for the life of the process).  src must be 16-byte
 * aligned, dst 4-byte aligned, crop * 3 a multiple of 4, n <= 65535.  Byte-identical to Pillow 12.x on the committed fixture tests/golden/ref_resize.npz
 * (Pillow's own outputs for seeded images of nine geometries) and on tests/golden/ref_resize_paths.json (every tap-count
 * instantiation, the buffer's last partial 16-byte piece, short last tiles, other resize / crop pairs, both sides of the size
 * bound below); torchvision is not importable where this is
 * built, so its output-size and crop-offset rules are restated.
 * Size bound: a workgroup keeps the intermediate rows of its 16 output rows in LDS, so large images are refused
 * (TTNET_E_UNSUPPORTED, beyond about 2650 px on the shorter side at resize 256 / crop 224: 2592 x 3888 is accepted,
 * 2848 x 4288 is not).  ttnet_resize_center_crop_u8_ragged has no such bound below 8192 px. */
int ttnet_resize_center_crop_u8(const uint8_t *src_hwc_dev, int64_t n, int h, int w, int resize, int crop,
                                uint8_t *dst_hwc_dev, void *stream);

/* Image i of a ragged batch: uint8 HWC [h][w][3] at byte `offset` of the source buffer (no alignment asked). */
typedef struct ttnet_image_desc {
  int64_t offset;
  int32_t h, w;
} ttnet_image_desc;                                   /* 16 bytes */

/* The same Resize(resize) + CenterCrop(crop), byte for byte, on a RAGGED batch: n images of any mix of sizes in one
 * buffer [src_dev, src_dev + src_bytes), described by n descriptors in DEVICE memory -> uint8 [n][crop][crop][3] in
 * descriptor order.  One kernel launch, asynchronous on `stream`; nothing is allocated, uploaded or waited for on the
 * host, and nothing is cached per geometry: every workgroup reads its image's descriptor and computes the output
 * size, the crop offsets and Pillow's coefficient tables itself (float64, in the order Pillow computes them), so the
 * call can be captured into a graph and replayed with new buffer contents, new geometries included.
 *   - src_dev 16-byte aligned, desc_dev 8-byte aligned, dst_dev 4-byte aligned, crop * 3 a multiple of 4,
 *     resize >= crop (no image can then fall short of the crop), 1 <= n <= 65535.
 *   - max_h / max_w bound every image's h / w; they size the LDS of a workgroup (which does not grow with the
 *     scale factor beyond the coefficient tables: about 100 KB at 8192 x 8192, resize 256 / crop 224).  Bounds
 *     the kernel cannot serve are refused here with TTNET_E_UNSUPPORTED (at 256 / 224: min(max_h, max_w) = 9274 is
 *     accepted and 9275 is not -- a staged input row of the crop must fit 6 x 256 16-byte pieces;
 *     tests/test_resize_paths_cpu.py derives it); an image is never refused on its own.  Crops other than 224 (up to 684,
 *     three dword columns per thread) are pinned to Pillow by tests/golden/ref_resize_paths.json.
 *   - a descriptor with h outside [1, max_h], w outside [1, max_w], a negative offset or bytes ending past
 *     src_bytes yields a zero crop and is counted in *bad_dev (int32, device memory, added to, never cleared) when
 *     bad_dev is not NULL.  Whatever the descriptors hold, the kernel reads nothing outside the source buffer and
 *     writes nothing outside dst. */
int ttnet_resize_center_crop_u8_ragged(const uint8_t *src_dev, int64_t src_bytes, const ttnet_image_desc *desc_dev,
                                       int64_t n, int max_h, int max_w, int resize, int crop, uint8_t *dst_dev,
                                       int32_t *bad_dev, void *stream);

/* Views: crops of a ragged batch other than the one centre crop -- corner crops, mirrored crops, boxes the caller chose.
 * A view is one crop x crop output cut from one image.  Its 48-byte descriptor is int32[12] =
 * {image, flags, bx, by, bw, bh, nw, nh, x0, y0, 0, 0}; arrays of them are 16-byte aligned.  Its pixels:
 *     B   = img[image][by : by + bh, bx : bx + bw]            the box, in source pixels
 *     R   = Pillow's BILINEAR resize of B to (nw, nh)         8-bit, horizontal pass then vertical pass, a pass skipped
 *                                                             when that size is unchanged (as ttnet_resize_center_crop_u8)
 *     out = R[y0 : y0 + crop, x0 : x0 + crop]                 columns reversed when flags & 1
 * The flip acts on the output window: it is hflip AFTER the resize, as in TenCrop and RandomHorizontalFlip.
 * A view is valid iff 0 <= image < n_images; that image's descriptor is valid (1 <= h, w <= 65536, its bytes inside the
 * buffer); the box lies inside the image with bw, bh >= 1; 1 <= nw, nh <= 65536; 0 <= x0, x0 + crop <= nw, likewise y0;
 * flags has no bit but bit 0 and the two reserved words are zero; bw / nw and bh / nh do not exceed the call's max_scale. */
typedef struct ttnet_view_desc {
  int32_t image, flags;
  int32_t bx, by, bw, bh;
  int32_t nw, nh;
  int32_t x0, y0;
  int32_t reserved[2];
} ttnet_view_desc;                                    /* 48 bytes */
#define TTNET_VIEW_FLIP 1                             /* flags */

/* n_views views of the n_images images of a ragged batch (buffer and image descriptors as for
 * ttnet_resize_center_crop_u8_ragged; view descriptors in DEVICE memory) -> uint8 [n_views][crop][crop][3] in view order.
 * Several views may name the same image.  One kernel launch -- the ragged kernel's own staging, horizontal pass and
 * vertical fold, handed another geometry -- asynchronous on `stream`; nothing is allocated, uploaded or cached, so the
 * call can be captured into a graph and replayed with new images and new descriptors.
 *   - src_dev and view_desc_dev 16-byte aligned, image_desc_dev 8-byte aligned, dst_dev 4-byte aligned, crop * 3 a
 *     multiple of 4, 1 <= n_images, n_views <= 65535.
 *   - max_scale >= 1 bounds bw / nw and bh / nh of every view: it sizes the coefficient tables and the staged input row
 *     as max_h / max_w do for the centre crop.  Bounds the 160 KB of LDS or the staging area cannot serve are
 *     TTNET_E_UNSUPPORTED (nothing launched).
 *   - an invalid view yields a zero crop and adds 1 to *bad_dev (when not NULL), once per view.  Whatever the
 *     descriptors hold, nothing outside [src_dev, src_dev + src_bytes) is read and a view writes only its own crop. */
int ttnet_resize_views_u8_ragged(const uint8_t *src_dev, int64_t src_bytes, const ttnet_image_desc *image_desc_dev,
                                 int64_t n_images, const ttnet_view_desc *view_desc_dev, int64_t n_views, double max_scale,
                                 int crop, uint8_t *dst_dev, int32_t *bad_dev, void *stream);

/* The evaluation families of views, written ON THE DEVICE from the image descriptors (those of
 * ttnet_jpeg_decode_ragged for instance: the host need not know any size): V descriptors per image, image-major (view
 * i * V + v).  The box is the whole image and (nw, nh) follow torchvision's Resize(resize), the rule of
 * ttnet_resize_center_crop_u8.  With mx = nw - crop, my = nh - crop, cx = round_half_even(mx / 2), cy likewise, the windows
 * (x0, y0, flip) are
 *     TTNET_VIEWS_CENTER  V = 1   (cx, cy, 0)                                          Resize + CenterCrop
 *     TTNET_VIEWS_FLIP    V = 2   (cx, cy, 0), (mx - cx, cy, 1)                        .. and the centre crop of the mirrored image
 *     TTNET_VIEWS_FIVE    V = 5   (0, 0, 0), (mx, 0, 0), (0, my, 0), (mx, my, 0), (cx, cy, 0)            FiveCrop
 *     TTNET_VIEWS_TEN     V = 10  FIVE, then (mx, 0, 1), (0, 0, 1), (mx, my, 1), (0, my, 1), (mx - cx, cy, 1)   TenCrop
 * (with an odd margin the mirrored image's centre crop is not the mirror of the centre crop).  An image with h < 1 or
 * w < 1 -- one that was not decoded -- gets invalid views.  resize >= crop; n_images * V <= 65535; image_desc_dev 8-byte,
 * view_desc_dev 16-byte aligned.  One launch, asynchronous, capturable.
 * ttnet_eval_views_max_scale is the max_scale these families need for images within max_h x max_w (host arithmetic only;
 * ttnet_resize_center_crop_u8_ragged sizes itself by the same function). */
enum { TTNET_VIEWS_CENTER = 0, TTNET_VIEWS_FLIP = 1, TTNET_VIEWS_FIVE = 2, TTNET_VIEWS_TEN = 3 };
int ttnet_make_eval_views(const ttnet_image_desc *image_desc_dev, int64_t n_images, int resize, int crop, int family,
                          ttnet_view_desc *view_desc_dev, void *stream);
double ttnet_eval_views_max_scale(int max_h, int max_w, int resize);

/* The mean of the views' outputs, torchvision's `outputs.view(n, V, -1).mean(1)`:
 *     out[i][c] = float32((sum over v of double(logits[i * V + v][c])) / V)
 * logits_dev float32 [n * V][C] -> out_dev float32 [n][C]; the sum in ascending v, in float64, so the result does not
 * depend on the launch; NaN propagates; V = 1 copies.  1 <= V <= 32, 1 <= n, n * V <= 65535 * 32, 1 <= C <= 65536; both
 * 4-byte aligned.  One launch, asynchronous, no allocation, capturable.  (The mean of the probabilities is left out.) */
#define TTNET_VIEWS_MAX 32
int ttnet_mean_views(const float *logits_dev, int64_t n, int64_t V, int64_t C, float *out_dev, void *stream);

/* JPEG decoding in front of the ragged resize: PIL.Image.open(path).convert("RGB"), the default loader of
 * torchvision.datasets.ImageFolder (main.py:208) that feeds the eval transform (utils/preprocess.py:104), on a batch of
 * compressed files.  Decoded on the device: Huffman-coded sequential 8-bit JPEG (SOF0, SOF1) with one scan holding
 * every component -- YCbCr (3 components, luma sampling 1x1 / 2x1 / 2x2, chroma 1x1) or greyscale (1 component,
 * replicated to RGB) -- with or without restart intervals, 1 <= h, w <= 8192.  The output is byte for byte what Pillow
 * 12.x with libjpeg-turbo 3.x decodes (islow integer IDCT, fancy upsampling, SCALEBITS 16 colour tables; the fixtures
 * under tests/golden/jpeg pin it).  Any other file is decoded on the host and carried as raw pixels (kind 1) that the
 * device copies through.
 *
 * Image i of the batch, built on the host from the markers before SOS (scale_imagenet_amd/jpeg.py, pack_jpeg); 80
 * bytes, the array 16-byte aligned.  kind 0 (decoded on the device): [data_offset, + data_bytes) of the source buffer is
 * the entropy-coded data after the SOS header, up to the end of the file; table_offset is a 2048-byte table block:
 * uint16 quant[3][64] (per frame component, zig-zag order as in DQT) at 0, then for component c = 0..2 the DC and
 * then the AC Huffman table of its scan as DHT holds them, counts[16] + symbols[256] (272 bytes each) at
 * 384 + 272 * (2c + ac).  comp[c] = {id, h_samp << 4 | v_samp, quant table, dc << 4 | ac table} (informative: the
 * block already holds the selected tables).  block_offset: first of this image's coefficient blocks (MCU columns x MCU
 * rows x blocks per MCU) in the decoder's workspace.  kind 1: data_offset holds uint8 HWC [h][w][3].  All kinds: the
 * decoded image goes to [out_offset, + h * w * 3) of dst.
 *
 * kind 2 (opt-in: pack_jpeg(..., progressive=True)): a complete Huffman-coded progressive file (SOF2), 8-bit, same
 * colour spaces, samplings and sizes as kind 0, with or without restart intervals, at most TTNET_JPEG_MAX_SCANS scans.
 * The host walks every scan and validates the progression as libjpeg's jdphuff.c does (T.81 G.1.1.1).  Refused there,
 * hence decoded on the host: a progression that leaves any coefficient of any component short of bit 0 (libjpeg would
 * smooth such blocks), a scan without data, an SOS naming an undefined table, an AC scan before the component's DC scan
 * or with several components, a refinement whose Ah is not the previous Al, quantisation tables redefined between
 * scans, more scans than the bound, SOF10, 12-bit, 4 components, DNL.  Layout: the 2048-byte table block at table_offset
 * holds quant[3][64] at 0 as for kind 0 and, at byte reserved[1] (>= 384, a multiple of 4), reserved[0] & 255 records of
 * ttnet_jpeg_scan in file order; (reserved[0] >> 16) & 255 Huffman tables of 272 bytes (counts[16] + symbols[256])
 * follow the block at table_offset + 2048, each distinct table of the file once; (reserved[0] >> 8) & 255 is the number
 * of rounds of the scans' schedule.  [data_offset, + data_bytes) is the file from the first scan's entropy-coded data to
 * the end of the last scan's; restart_interval is the first scan's (informative).  block_offset and the block count are
 * those of a sequential file of the same frame.  With the flag off, and for every other file, nothing changes. */
#define TTNET_JPEG_MAX_SCANS 32   /* libjpeg-turbo's default script has 10 scans for colour, 6 for greyscale */
typedef struct ttnet_jpeg_desc {
  int64_t data_offset, data_bytes;
  int64_t table_offset;
  int64_t out_offset;
  int64_t block_offset;
  int32_t h, w;
  int32_t kind;              /* 0: sequential JPEG decoded on the device, 1: raw pixels copied, 2: progressive JPEG */
  int32_t ncomp;             /* 1 or 3 */
  int32_t restart_interval;  /* MCUs per restart segment, 0: none */
  uint8_t comp[3][4];
  int32_t reserved[2];       /* kind 2: {scans | rounds << 8 | Huffman tables << 16, scan list offset}; else 0 */
} ttnet_jpeg_desc;

/* One scan of a kind-2 image, 32 bytes.  [data_offset, + data_bytes) is its entropy-coded data relative to the image's
 * data_offset (up to the next marker that is not FF00 / RSTn).  comp: frame component indices, increasing; a scan of one
 * component covers that component's own ceil(w_c / 8) x ceil(h_c / 8) blocks and its restart interval counts blocks, a
 * scan of several covers the frame's MCUs.  table[q]: index into the image's Huffman pool of the table in force for
 * scan component q when the SOS was read (the DC table in a DC first pass, table[0] the AC table in an AC scan; unused
 * in a DC refinement).  slot = 4 * round + wave: scans of one round are decoded side by side, and a scan's round comes
 * after the round of every earlier scan that codes one of its (component, coefficient) pairs. */
typedef struct ttnet_jpeg_scan {
  uint32_t data_offset, data_bytes;
  uint16_t restart_interval;  /* blocks or MCUs per restart segment in this scan, 0: none */
  uint8_t ncomp;              /* components in the scan: 1 .. 3 (AC scans: 1) */
  uint8_t slot;
  uint8_t comp[4];
  uint8_t ss, se, ah, al;     /* spectral band Ss .. Se (DC: 0, 0), successive approximation Ah, Al */
  uint8_t table[4];
  int32_t reserved[2];
} ttnet_jpeg_scan;

typedef struct ttnet_jpeg_ctx ttnet_jpeg_ctx;

/* A decoder context on `device`; its workspace is sized by ttnet_jpeg_ctx_reserve (the only calls that allocate). */
int ttnet_jpeg_ctx_create(int device, ttnet_jpeg_ctx **out);
/* Sizes the workspace for batches of up to max_images images, max_blocks coefficient blocks in all and max_bytes bytes of
 * source buffer (about 128 bytes per block + 19 bytes per source byte; progressive images use the same coefficient blocks
 * and nothing more).  Replaces (and frees) the previous workspace:
 * call it outside graph capture, with no decode in flight on the context. */
int ttnet_jpeg_ctx_reserve(ttnet_jpeg_ctx *ctx, int64_t max_images, int64_t max_blocks, int64_t max_bytes);
/* Decodes n images described by jdesc_dev (device memory) from [src_dev, src_dev + src_bytes) into dst_dev, back to back
 * at each descriptor's out_offset, and writes their ttnet_image_desc records (out_offset, h, w) to dst_desc_dev: the
 * input of ttnet_resize_center_crop_u8_ragged.  n_blocks is the descriptors' total of coefficient blocks.  Four kernel
 * launches on `stream` whatever the batch holds (the progressive kernel leaves at once for images of kind 0 and 1); nothing is allocated, copied or waited for, nothing is cached per image, so the call can be
 * captured into a graph and replayed with new images within the same reservation.  TTNET_E_INVALID when n, n_blocks or
 * src_bytes exceed the reservation.  src_dev and jdesc_dev 16-byte aligned, dst_desc_dev 8-byte aligned.
 *   - corrupt entropy-coded data (truncated, a bad Huffman code, a coefficient index past 63, a missing or misnumbered
 *     RST; in a progressive scan also data that runs out, a coefficient index past Se, an end-of-band run past the
 *     scan's last block) makes that image all zero and adds 1 to stats_dev[0]; a descriptor or scan record outside the
 *     buffers or the reservation does too, and its output record gets h = w = 0.  The kernels read nothing outside the source buffer and write
 *     nothing outside the workspace and each image's own output span, whatever the bitstream holds.
 *   - stats_dev[1] (int32, added to) counts restart segments whose subsequence synchronisation was still changing after
 *     its round bound and that were then walked sequentially (per segment; the settled segments of the same image are
 *     not).  TTNET_JPEG_SEQUENTIAL=1 walks every segment so and counts them all (diagnostic: the result is the same).
 *     Progressive images are not counted here and ignore the switch.
 *   - the workspace (ttnet_jpeg_ctx_reserve) is baked into a captured graph: it must not be re-reserved while such a
 *     graph may still be replayed. */
int ttnet_jpeg_decode_ragged(ttnet_jpeg_ctx *ctx, const uint8_t *src_dev, int64_t src_bytes,
                             const ttnet_jpeg_desc *jdesc_dev, int64_t n, int64_t n_blocks, uint8_t *dst_dev,
                             int64_t dst_bytes, ttnet_image_desc *dst_desc_dev, int32_t *stats_dev, void *stream);
void ttnet_jpeg_ctx_destroy(ttnet_jpeg_ctx *ctx);

/* Evaluation metrics on the device: replaces `loss = criterion(outputs, targets)`, `accuracy(outputs, targets, (1, 5))`
 * and the three AverageMeter.update calls of test() (main.py:262-268; utils/bar_show.py:110-148) with one call that keeps
 * nothing but this accumulator.  The call ADDS to it, so one accumulator per lane (zeroed by the caller, 8-byte aligned,
 * device memory) collects a whole evaluation and is read back once: loss = loss_sum / images, Acc@k = 100 * hitsk / images. */
typedef struct ttnet_eval_acc {
  double loss_sum;      /* sum of the per-image losses (float64) */
  int64_t images;       /* rows with a valid target */
  int64_t hits1, hits5;
  int64_t bad_targets;  /* rows whose target was outside [0, n_classes) */
  int64_t reserved[3];
} ttnet_eval_acc;       /* 64 bytes */

/* logits_dev float32 [n][n_classes] contiguous (any 4-byte aligned address), targets_dev int64 [n]; n in [1, 65535],
 * n_classes in [2, 65536].  Per row, with v = the row, t = its target:
 *   loss = logsumexp(v) - v[t], evaluated in float64 from the float32 logits: log(sum_j exp(v_j - max v)) + max v - v_t,
 *          the sum taken in a fixed lane / tree order.
 *   rank = #{j : v_j > v_t} + #{j < t : v_j == v_t}; the image is a top-k hit iff rank < k.  This is the reference's
 *          topk-based accuracy whenever the target's logit is not tied across the k-th place; torch.topk leaves the order
 *          of ties unspecified, so ties are DEFINED here to go to the lower class index.
 *   A NaN anywhere in the row: loss = NaN (and so the accumulator's loss_sum), no hit; rank is recorded as INT32_MAX.
 *   t outside [0, n_classes): no hit, nothing added to loss_sum or images, bad_targets + 1; rank is recorded as -1, loss
 *          as 0.  The row is never indexed with such a target.
 * per_image_dev, when not NULL, receives n records {double loss; int32 rank; int32 zero} (16 bytes each, 8-byte aligned)
 * and is the buffer the reduction reads.  The reduction is deterministic: the records are summed in a fixed order (a
 * fixed stride over the images, then a fixed tree) by one workgroup and added to the accumulator by one thread; no
 * floating-point atomics, so the same batches in the same order give the same bits run to run.
 * Two launches on `stream`; no plan, no host synchronisation, capturable in a graph.  With per_image_dev there is no
 * allocation either; with NULL the library keeps one 1 MiB scratch per accumulator address, allocated by the first call
 * that names that accumulator (which must therefore not be a capturing one: TTNET_E_STATE) and kept for the life of the
 * process, at most 64 of them.  Calls that add to one accumulator must be ordered by their stream. */
int ttnet_eval_metrics(const float *logits_dev, const int64_t *targets_dev, int64_t n, int64_t n_classes,
                       ttnet_eval_acc *acc_dev, void *per_image_dev, void *stream);

/* Per-image predictions: the k best classes of every row, best first.  logits_dev as for ttnet_eval_metrics (float32
 * [n][n_classes] contiguous, any 4-byte aligned address; n in [1, 65535], n_classes in [2, 65536]); k in
 * [1, min(n_classes, TTNET_TOPK_MAX)].  topk_dev (8-byte aligned) receives n * k records of 16 bytes,
 * {int32 class; float32 logit; double logprob}, row after row.  Per row, with v = the row:
 *   order    larger logit first; equal logits go to the lower class index -- the tie rule of ttnet_eval_metrics, so slot
 *            r of a row holds the class whose rank there is r.  -inf logits are ordinary values (they come last, lower
 *            index first); -0 and +0 are equal.
 *   logprob  = -(log(sum_j exp(v_j - max v)) + max v - v_class) in float64, the sum taken in the same lane / tree order
 *            as ttnet_eval_metrics takes it (one piece of code): bit for bit the negative of the loss that call records
 *            for a row whose target is that class.
 *   A NaN anywhere in the row: every slot gets class -1, logit NaN, logprob NaN (rank INT32_MAX there).
 * Deterministic: the same input gives the same bytes, run to run.  One launch on `stream`; no plan, no host
 * synchronisation, no allocation, capturable in a graph.  TTNET_E_INVALID (nothing launched) for a NULL pointer, n,
 * n_classes or k outside their ranges, k > n_classes, or a misaligned buffer. */
#define TTNET_TOPK_MAX 32
int ttnet_topk_rows(const float *logits_dev, int64_t n, int64_t n_classes, int64_t k, void *topk_dev, void *stream);

/* Per-class counters from a batch that ttnet_eval_metrics and ttnet_topk_rows have seen: targets_dev int64 [n],
 * per_image_dev the n per-image records of ttnet_eval_metrics, topk_dev the n * k records of ttnet_topk_rows (only slot
 * 0, the top-1 class, is read).  ADDS into counts_dev, int64 [n_classes][4] = {images, hits1, hits5, predicted}, and,
 * when confusion_dev is not NULL, into int64 [n_classes][n_classes] indexed [target][top-1 class]; both zeroed by the
 * caller, 8-byte aligned.  Per row, following the accumulator of ttnet_eval_metrics:
 *   target outside [0, n_classes) (rank -1): the row is left out of everything.
 *   otherwise images[target] + 1, hits1[target] + 1 if rank == 0, hits5[target] + 1 if rank < 5; predicted[class] + 1 and
 *   confusion[target][class] + 1 for the row's top-1 class.  A row with a NaN (rank INT32_MAX, class -1) is an image
 *   without a hit, as it is there, and predicts nothing: it adds to images[target] only.
 * So the column sums of counts over the classes are the accumulator's images, hits1, hits5, and predicted sums to the
 * rows without a NaN.  Integer atomic adds only: the result does not depend on the order of the rows, of the calls, or
 * of the streams that add to the same counters.  One launch on `stream`; no synchronisation, no allocation,
 * capturable.  Argument ranges as for ttnet_topk_rows; TTNET_E_INVALID otherwise (nothing launched). */
int ttnet_class_counts(const int64_t *targets_dev, const void *per_image_dev, const void *topk_dev, int64_t n, int64_t k,
                       int64_t n_classes, int64_t *counts_dev, int64_t *confusion_dev, void *stream);

/* Same, starting from the binarised stem output (features[3], netbin.py:193) given as
 * row-packed bits uint64 [n][p][56]; used by the parity tests to separate the integer
 * gate path (bit exact) from the float stem (exact except at near ties). */
int ttnet_forward_from_stem_bits(ttnet_plan *plan, const uint64_t *rows_dev, int64_t n,
                                 float *logits_dev, void *stream);

/* Parity taps: copies a stage of the LAST forward on this plan to `dst` (host pointer
 * unless on_device).  Stages: "features.3", "features.4", "features.5" (row-packed uint64
 * [n][C][H]), "features.<b>.out1".."out4" (row-packed, after the branch padding),
 * "flatten" (float32 [n][fcsize] in the reference's C-major order), "stem.pre"
 * is not kept.  Synchronises `stream`.  Replaces the reference's debug attributes
 * Block_TT.input_layer / output_layer (models/TT_FHE_SMALL.py:310,319). */
int ttnet_read_stage(ttnet_plan *plan, const char *stage, int64_t n, void *dst, size_t dst_bytes,
                     int on_device, void *stream);

/* Truth-table export / import in the reference's canonical order
 * (Block_TT.get_TT_block_all_filter, models/TT_FHE_SMALL.py:322-342): for Block_TT `name`
 * (e.g. "features.4.Block_conv3"), `bits` is uint8 [groups][2^n][cout_per_group] with
 * entry index = the pattern read MSB first over (c_in_group, kh, kw).  get copies the
 * table the plan built; set replaces it (e.g. with truth tables published alongside a
 * checkpoint, README.md:22).  For the last (float) block the element type is float32. */
int ttnet_plan_get_table(ttnet_plan *plan, const char *name, void *dst_host, size_t dst_bytes);
int ttnet_plan_set_table(ttnet_plan *plan, const char *name, const void *src_host, size_t src_bytes);

/* Truth-table usage counts: which entries of the tables a forward actually read.  For Block_TT `name` with G groups
 * and n input bits, usage is int64 [G][2^n] in the canonical order of ttnet_plan_get_table (index = pattern read MSB
 * first over (c_in_group, kh, kw), convolution zero padding = bit 0): usage[g][i] = number of (image, output position)
 * pairs at which the input window of group g had index i.  Output positions are all Ho x Wo positions of the block's own
 * convolution, those a later floor-cropped majority pool discards included; Block_convf reads the interleaved,
 * branch-padded concat (channel 4c + branch, the zero pads are bit 0).  So usage[g].sum() == images * Ho * Wo for every g.
 *   enable  allocates and zeroes one int64 counter per table entry of the plan (543 MB for TT-small p = 64 --layers 1) and
 *           the per-lane scratch of the add (ttnet_plan_set_lanes grows it with the lanes); enabled = 0 frees both.
 *           Synchronises the device: call it outside graph capture.  "usage_bytes" (ttnet_plan_query) is what it holds.
 *   reset   zeroes the counters, asynchronously on `stream`.
 *   add     adds the lookups of the forward last issued on `lane` (all of its images), whichever entry point issued it
 *           (ttnet_forward, _lane, _u8, _from_stem_bits) and whether it ran as plain launches or as a replayed graph: it
 *           reads the stage buffers the lane still holds.  Asynchronous on `stream`; the caller orders it after that
 *           lane's forward and before the lane is reused.  Its own launches only (the forward kernels do not change); no
 *           allocation, no host synchronisation.  On the block-fused path the branch tensors never reach memory, so every
 *           non-last block is run once more with a tap buffer, as ttnet_read_stage does.  64-bit integer atomics: the
 *           counts do not depend on batch order, lane, stream or rank.
 *   get     synchronises the device and copies the counters of one block to the host (dst_bytes = G * 2^n * 8).
 * Errors: add / reset / get before enable TTNET_E_STATE; an unknown block name or a wrong dst_bytes TTNET_E_INVALID.
 * Served: TTNET_SMALL (every built p and --layers, fused and two-launch gate paths) and TTNET_XSMALL.  Refused by enable
 * with TTNET_E_UNSUPPORTED: TTNET_FULL (fan-in 30: no tables, the reason ttnet_plan_get_table gives) and TTNET_VALEXNET
 * (not built: its block has no Block_convf and its own stage layout). */
int ttnet_plan_table_usage_enable(ttnet_plan *plan, int enabled);
int ttnet_plan_table_usage_reset(ttnet_plan *plan, void *stream);
int ttnet_table_usage_add(ttnet_plan *plan, int lane, void *stream);
int ttnet_plan_get_table_usage(ttnet_plan *plan, const char *name, int64_t *dst_host, size_t dst_bytes);

/* Care-set misses: per image, how many lookups of a forward fell outside a chosen set of table entries.  A care set for
 * Block_TT `name` (G groups, n input bits) is a bitmap uint32 [G][max(1, 2^n / 32)]: entries in the canonical order of
 * ttnet_plan_get_table, bit i % 32 of word i / 32 = entry i of the group, unused high bits zero (the bitmap format of
 * ttnet_minimise_covers).  A miss is a lookup whose entry has bit 0.  The lookups are those ttnet_table_usage_add counts:
 * every Ho x Wo output position of the block's own convolution, positions a later floor-cropped pool discards included.
 * An image without a miss in any block gets the same stage bits, hence bit-identical logits, from ANY tables that agree
 * with the plan's on the care sets -- e.g. a circuit minimised with the other entries as don't-cares.
 *   set_care     installs or replaces the bitmap of one block (bytes = G * max(1, 2^n / 32) * 4); bits_host == NULL removes
 *                it.  The first install also allocates the per-lane scratch of ttnet_table_usage_add (ttnet_plan_set_lanes
 *                grows it with the lanes), never the usage counters: care sets and usage counts are independent, on together
 *                or separately, and share that scratch.  Synchronises the device: call it outside graph capture.
 *   clear_care   removes every bitmap, and frees the scratch unless the usage counters are on.
 *   care_misses  rows_dev = int32 [n][B] for the n images of the forward last issued on `lane` (whichever entry point issued
 *                it, plain launches or a replayed graph), B = ttnet_plan_query("care_blocks") = the Block_TTs of the plan in
 *                the order conv1, conv2, conv3, convf per block: rows_dev[i][b] = misses of image i in Block_TT b, 0 for a
 *                block without a bitmap.  It zeroes the rows itself.  Asynchronous on `stream`, ordered by the caller after
 *                that lane's forward and before the lane is reused; its own launches only, no allocation, no host
 *                synchronisation, capturable.  On the block-fused path every non-last block whose convf has a bitmap is run
 *                once more with a tap buffer, as the usage add does.  int32 adds only: the rows do not depend on launch
 *                geometry, lane or stream.
 * "care_bytes" (ttnet_plan_query) is what the bitmaps hold; the shared scratch is part of "usage_bytes" while either
 * feature is on.  Errors: care_misses before any set_care (or after clear_care) and a lane without a forward TTNET_E_STATE;
 * a bad lane, a NULL or misaligned rows_dev, an unknown block name, a wrong `bytes` TTNET_E_INVALID.  Served and refused
 * variants (TTNET_E_UNSUPPORTED from set_care) as for ttnet_plan_table_usage_enable. */
int ttnet_plan_set_care(ttnet_plan *plan, const char *name, const uint32_t *bits_host, size_t bytes);
int ttnet_plan_clear_care(ttnet_plan *plan);
int ttnet_care_misses(ttnet_plan *plan, int lane, int32_t *rows_dev, void *stream);

/* Two-level minimisation of truth tables with don't-cares, on the device: a PRIME and IRREDUNDANT cover of every
 * function of a batch (every cube is a prime implicant of ON u DC, no cube can be removed).  It is not a minimum cover.
 *
 * A function of n_bits inputs (1..16) is two bitmaps over its 2^n patterns, indexed in the canonical order of
 * ttnet_plan_get_table (variable x_j is index bit n-1-j): `on`, where it must be 1, and `dc`, where it may take either
 * value (a pattern in both counts as ON); OFF is the rest.  A cube is (mask, value): mask = the n-bit set of index bits
 * that carry a literal, value & ~mask == 0, packed as the uint32 key mask << 16 | value; it holds the patterns p with
 * p & mask == value.  The cover is defined by four steps, which the device code and scale_imagenet_amd.minimise's CPU
 * twin both follow, so that they give the same keys in the same order:
 *   1 expand       for every ON minterm m on its own: start from the cube with all n literals of m; for j = 0 .. n-1 in
 *                  that order drop the literal of x_j iff the sibling half (the current cube with x_j complemented)
 *                  holds no OFF pattern.  One pass leaves a prime: a cube only grows, so a refused drop stays refused.
 *   2 order        the candidates by number of free variables, descending, then by generating minterm, ascending.
 *   3 cover        walk that order; keep a cube iff it holds an ON minterm that no kept cube holds yet (duplicates drop
 *                  out by themselves).
 *   4 irredundant  walk the kept cubes in reverse; remove a cube iff every ON minterm in it also lies in another cube
 *                  that is still kept.
 * The output is the surviving cubes in the order of step 2.  An empty ON set gives no cube (constant 0); otherwise an
 * empty OFF set gives the one cube with the empty mask, key 0 (constant 1).  The CNF of a function is the same
 * procedure on on' = ~on & ~dc with the same dc, read by De Morgan: every cube becomes a clause of complemented literals.
 *
 * on_dev / dc_dev: uint32 [n_funcs][max(1, 2^n / 32)], bit i%32 of word i/32 is pattern i (unused high bits zero);
 * dc_dev may be NULL (no don't-cares).  cubes_dev: uint32 [n_funcs][cube_cap] keys; counts_dev: int32 [n_funcs], the
 * TRUE number of cubes of each cover.  The cap rule: cubes past cube_cap are not written, the caller sees
 * counts > cube_cap and calls again; a cap >= the function's ON count never overflows; cube_cap 0 asks for the counts
 * alone.  work_dev / work_bytes: scratch, at least ttnet_minimise_workspace(n_bits, n_funcs) bytes (8 * 2^n bytes,
 * rounded up to 256, for each of min(n_funcs, 1024) workgroups), 16-byte aligned; the other buffers 4-byte aligned.
 * One launch on `stream`: no plan, no host synchronisation, no allocation, capturable in a graph; integers only, so the
 * same input gives the same bytes.  TTNET_E_INVALID (nothing launched) for a NULL pointer other than dc_dev, n_bits
 * outside 1..16, n_funcs < 1, cube_cap < 0, a misaligned buffer or a workspace that is too small;
 * ttnet_minimise_workspace returns TTNET_E_INVALID for arguments outside those ranges. */
int64_t ttnet_minimise_workspace(int n_bits, int64_t n_funcs);
int ttnet_minimise_covers(const uint32_t *on_dev, const uint32_t *dc_dev, int n_bits, int64_t n_funcs,
                          uint32_t *cubes_dev, int64_t cube_cap, int32_t *counts_dev,
                          void *work_dev, int64_t work_bytes, void *stream);

/* The same covers made smaller by `rounds` (0..8) reduce / expand rounds on the device; everything said above holds, and
 * rounds = 0 gives the bytes of ttnet_minimise_covers.  Round 0 is the four steps and yields the cover K_0, an ordered list
 * of keys.  Round r = 1 .. rounds turns K_{r-1} into K_r:
 *   5 count        for every ON pattern, how many cubes of K_{r-1} hold it (what step 4 left behind).
 *   6 reduce       walk the cubes of K_{r-1} from the last to the first.  E = the ON patterns of cube c whose count is 1;
 *                  E is never empty, because K_{r-1} is irredundant and a count only falls for patterns that a cube
 *                  leaves.  Replace c by the smallest cube that holds E (mask = the index bits on which all of E agree,
 *                  value = their common bits) and decrement the count of every ON pattern of c that the smaller cube no
 *                  longer holds.  Sequential by definition: the cubes walked later see the lowered counts.
 *   7 expand       every reduced cube on its own, as in step 1, to a prime again; it keeps its position.  The literals
 *                  are tried in the order x_{n-1} .. x_0 when r is odd and x_0 .. x_{n-1} when r is even.
 *   8 order        by number of free variables, descending, then by position in K_{r-1}, ascending; then steps 3 and 4
 *                  unchanged (a repeated key drops out in step 3 by itself).  The result is K_r.
 *   9 best         the call returns the K_r, r = 0 .. rounds, with the smallest (literals, cubes), compared in that
 *                  order; the earliest r wins a tie.  All rounds run, and round r+1 starts from K_r, not from the best.
 * So the result is prime and irredundant, never carries more literals than the cover of ttnet_minimise_covers, and is
 * deterministic.  A constant function and a K_0 of one cube are returned before any round.
 * work_dev: at least ttnet_minimise_rounds_workspace(n_bits, n_funcs) bytes for every `rounds`: 16 * 2^n bytes, rounded up
 * to 256, for each of min(n_funcs, 1024) workgroups (the 8 of ttnet_minimise_covers, a key list for the cover in hand and
 * one for the best).  TTNET_E_INVALID (nothing launched) also for rounds outside 0..8. */
int64_t ttnet_minimise_rounds_workspace(int n_bits, int64_t n_funcs);
int ttnet_minimise_covers_rounds(const uint32_t *on_dev, const uint32_t *dc_dev, int n_bits, int64_t n_funcs, int rounds,
                                 uint32_t *cubes_dev, int64_t cube_cap, int32_t *counts_dev,
                                 void *work_dev, int64_t work_bytes, void *stream);

/* Rule support: which cubes of a cover the data uses.  For each of n_funcs functions of n_bits inputs (1..16) it joins a
 * cover with the lookup counts of the function's table and says what every cube carries.
 *
 * cubes_dev uint32 [n_funcs][cube_cap], counts_dev int32 [n_funcs]: the keys and counts of ttnet_minimise_covers, in that
 * call's order (any list of keys will do; a cube holds pattern p iff p & mask == value).  Entries past counts[f] are never
 * read.  A counts[f] above cube_cap cannot be refused without a host synchronisation: the caller, who knows the counts,
 * checks it (scale_imagenet_amd.rules does); the kernel reads min(counts[f], cube_cap) cubes, a negative count as 0.
 * keep_dev uint8 [n_funcs][cube_cap] or NULL: cube c of function f is KEPT iff keep[f][c] != 0; NULL keeps every cube.
 * usage_dev int64 [n_usage_rows][2^n], usage_row_dev int32 [n_funcs]: function f weighs pattern p with
 * u[p] = usage_dev[usage_row_dev[f]][p], patterns in the canonical order of ttnet_plan_get_table; several functions may
 * share a row, as the output bits of a group do.
 *
 * Outputs, for function f over its kept cubes in their order (int64 [n_funcs][cube_cap]; a cube that is not kept and
 * every entry from counts[f] on get 0 in all three):
 *   hits[c]   the sum of u[p] over the patterns cube c holds;
 *   first[c]  the sum of u[p] over the patterns for which c is the first kept cube that holds them (the decision-list
 *             reading: a partition of the covered mass);
 *   sole[c]   the sum of u[p] over the patterns that c holds and no other kept cube holds: the lookups whose output bit
 *             changes if c alone is removed.
 * totals_dev int64 [n_funcs][4] = {covered, lost, used_patterns, lost_patterns}: covered, the mass of the patterns held by
 * at least one kept cube; lost, the mass of those held by a cube of the full list but by no kept cube; used_patterns, the
 * patterns with u > 0; lost_patterns, the number of lost patterns whatever their u.  lost_bits_dev, uint32
 * [n_funcs][max(1, 2^n / 32)] or NULL: the bitmap of the lost patterns in the format of ttnet_minimise_covers (unused
 * high bits zero).  With keep_dev NULL nothing is lost: lost, lost_patterns and the bitmap are zero.
 *
 * A usage_row_dev[f] outside [0, n_usage_rows) reads nothing from usage_dev: every output of function f is zero (its
 * hits / first / sole rows, its totals, its bitmap), and the number of such functions is left as an int64 in the first 8
 * bytes of work_dev, which the call sets to zero before anything else; the rest of the workspace is scratch.
 * work_dev / work_bytes: at least ttnet_cover_support_workspace(n_bits, n_funcs) bytes: 256 for that count, then 10 * 2^n
 * bytes, rounded up to 256, for each of min(n_funcs, 1024) workgroups.
 * A 256-byte memset and one launch on `stream`: no plan, no allocation, no host synchronisation, capturable in a graph.
 * Integer adds only: the bytes do not depend on the launch geometry.  Every element of the six outputs is written, so the
 * caller zeroes nothing.  TTNET_E_INVALID (nothing launched) for a NULL pointer other than keep_dev / lost_bits_dev, n_bits
 * outside 1..16, n_funcs < 1, cube_cap outside 1..2^31-1, n_usage_rows < 0, a misaligned buffer (4 bytes for cubes,
 * counts, rows and bitmap, 8 for the int64 buffers, 16 for the workspace) or a workspace that is too small;
 * ttnet_cover_support_workspace returns TTNET_E_INVALID for n_bits or n_funcs outside those ranges. */
int64_t ttnet_cover_support_workspace(int n_bits, int64_t n_funcs);
int ttnet_cover_support(const uint32_t *cubes_dev, const int32_t *counts_dev, int64_t cube_cap, const uint8_t *keep_dev,
                        const int64_t *usage_dev, const int32_t *usage_row_dev, int64_t n_usage_rows,
                        int n_bits, int64_t n_funcs,
                        int64_t *hits_dev, int64_t *first_dev, int64_t *sole_dev, int64_t *totals_dev,
                        uint32_t *lost_bits_dev, void *work_dev, int64_t work_bytes, void *stream);

/* Certified L-infinity robustness of TTNET_VALEXNET on the device (csrc/certify.hip; DESIGN.md: certified robustness).
 *
 * Question: does image i keep the class classes_dev[i] when every input byte may move by up to eps?  x_nhwc_dev is what
 * ttnet_forward_u8 takes: uint8 [n][32][32][3].  Every byte b may become any REAL value in [max(0, b - eps), min(255, b + eps)]
 * (eps >= 0 in byte levels: 2.0 is 2/255); ToTensor and Normalize follow with the plan's constants
 * (ttnet_plan_set_input_norm); the zero padding of the convolution stays zero in normalised space.  The answer is SOUND, not
 * complete: "certified" is never wrong about the exact-arithmetic network, but a robust image may stay uncertified.
 *
 *   stage 0  Interval arithmetic through conv3x3 + bias (lo = sum w+ x_lo + w- x_hi + bias over the taps inside the image,
 *            hi symmetrically), ReLU, eval BatchNorm (a negative scale swaps the bounds) and MaxPool(3) (max of the lows, max
 *            of the highs), in float64.  Each bound is then widened outward by the per-channel slack
 *              slack_c = 2^-40 ((|w_c|_1 X + |bias_c|) |scale_c| + |shift_c|),   X = max |normalised value| of the bytes 0..255,
 *            computed once on the host: over a hundred times what the ~60 float64 roundings behind a bound can add up to
 *            (2^-53 of operands of that size each), so the widened bounds hold for exact arithmetic whatever order and
 *            form the sums are taken in.  lo_bit = (lo >= 0), hi_bit = (hi >= 0):
 *            a stem bit is unknown where they differ; lo_bit <= hi_bit always.
 *   stage 1  The block on three-valued bits, exact per lookup: an output bit can be 1 iff a table entry compatible with the
 *            known inputs is 1 (likewise 0); paddings are known zeros; out4 carries the stem planes.  With the effective head
 *            A = lin2 diag(bn_scale) lin1 (float64, [10][30976] as a matrix; how the library stores it is internal and
 *            never crosses this interface), c0 = lin2 bn_shift + bias, and D = A_c - A_j:
 *              lb_j = c0_c - c0_j + sum_f D_f ylo_f + sum_{f unknown} min(0, D_f),   lb_interval = min_{j != c} lb_j,
 *            worst = the first j that attains it.
 *   stage 2  For an image that stage 1 left open and that has 1 <= k <= enum_bits unknown stem bits: the minimum over all 2^k
 *            completions of the unknown stem bits of min_{j != c} (logit_c - logit_j) (ties: the smaller j).  Still sound
 *            (the unknown bits are free), and free of the independence loss of stage 1.  enum_bits 0 switches it off.
 *
 * rows_dev receives n records of 32 bytes (8-byte aligned):
 *   { double lb_interval; double lb; int32 worst; int32 stage; int32 unknown_stem; int32 unknown_feat; }
 * lb = the enumerated bound when stage 2 ran, else lb_interval; stage = 1 certified by the interval bound, 2 certified by
 * enumeration, 0 not certified; certified means lb > min_margin.  The certificate speaks of the exact-arithmetic network;
 * the logits of ttnet_forward_u8 lie within the 1e-5-scaled tolerance of it, so a caller who wants the device's own argmax
 * certified passes min_margin = twice that tolerance.  A class outside 0..9 is NOT an error of the call (the classes live on
 * the device and nothing is read back): that image gets stage 0, worst -1 and lb = lb_interval = -inf.
 * planes_dev: NULL, or an 8-byte aligned buffer of n * (2 * 640 + 2 * 2816) uint64 that receives the stem planes lo, hi
 * ([n][64][10], layout of stage "features.4") and the feature planes lo, hi ([n][256][11], layout of "features.5"), in that order.
 *
 * Float64 sums in a fixed order and integer work: the same input gives the same bytes.  Launches on `stream`, not captured in a
 * graph by the plan; the lane's planes (55 KB per image of max_batch) are allocated by the first call on that lane, A, c0 and
 * the slack by the first call after a (re)load, which synchronises; forwards and their workspaces are untouched, so a certify
 * call and a forward on the same lane may overlap.  With profiling on, ttnet_plan_last_timings then reports the steps
 * "certify.stem", "certify.block", "certify.margin", "certify.enum" of this call.  Errors: eps negative or not finite, enum_bits outside 0..12, min_margin
 * NaN, a bad lane, n outside [1, max_batch], a NULL or misaligned pointer (4 bytes for images and classes, 8 for records and
 * planes) TTNET_E_INVALID; any variant other than TTNET_VALEXNET TTNET_E_UNSUPPORTED (the certificate needs an affine head
 * and truth tables of at most 8 inputs); before finalize TTNET_E_STATE. */
int ttnet_certify_u8(ttnet_plan *plan, int lane, const uint8_t *x_nhwc_dev, int64_t n, const int32_t *classes_dev, double eps,
                     int enum_bits, double min_margin, void *rows_dev, uint64_t *planes_dev, void *stream);

/* The same certificate for a box given per byte: byte k of image i may take any REAL value in [lo, hi], lo and hi being byte k of
 * lo_nhwc_dev and hi_nhwc_dev (uint8 [n][32][32][3] each, 4-byte aligned).  Where lo > hi the byte counts as the degenerate
 * box [lo, lo] (nothing is read back to refuse it; the Python wrappers refuse it).  Stage 0 takes the centre and the radius of
 * every pixel's interval from the two images where ttnet_certify_u8 takes them from b -+ eps: the same kernel, slack and
 * float64 order, so lo = max(0, b - e), hi = min(255, b + e) for an integer e gives the bytes of ttnet_certify_u8 at eps = e.
 * Stages 1 and 2, the records, planes_dev, the lane's buffers, the profiling steps and the errors are ttnet_certify_u8's
 * (without eps; hi_nhwc_dev NULL or misaligned is TTNET_E_INVALID). */
int ttnet_certify_box_u8(ttnet_plan *plan, int lane, const uint8_t *lo_nhwc_dev, const uint8_t *hi_nhwc_dev, int64_t n,
                         const int32_t *classes_dev, int enum_bits, double min_margin, void *rows_dev, uint64_t *planes_dev,
                         void *stream);

/* Certified PATCH robustness of TTNET_VALEXNET: every position of a patch_h x patch_w patch (1..8 each) in one call (DESIGN.md:
 * certified patch robustness).  Positions (y0, x0) = (a * stride, b * stride) with y0 + patch_h <= 32 and x0 + patch_w <= 32, row-major:
 * P = Py * Px, Py = (32 - patch_h) / stride + 1, Px likewise (stride 1..32).  The box of position p: the bytes of the patch's
 * pixels (all three channels) lie in [max(0, b - amp), min(255, b + amp)], amp an integer in 1..255 (255: any value); every
 * other byte is exact.  The record of (image, position) is what ttnet_certify_box_u8 gives for that box: the same three-valued
 * planes, the same integers, and lb equal as a real number -- computed incrementally:
 *   per image, once ("patch.base"): stages 0 and 1 on the degenerate box (a clean bit within the slack of zero stays unknown),
 *     which leave the clean planes and, per class j, S_j = sum_f D_f ylo_f and U_j = sum_{f unknown} min(0, D_f) in
 *     ttnet_certify_u8's order;
 *   per (image, position), one workgroup ("patch.sweep"): stage 0 for the pooled cells whose 5 x 5 pixel field (rows 3 py - 1 ..
 *     3 py + 3, likewise columns) meets the patch, at most 4 x 4 cells x 64 channels, by the code stage 0 runs; stage 1's lookups
 *     for the features those cells reach; for each such feature whose three-valued value differs from the clean one, the
 *     differences dS_j = D_f (ylo_f - clean ylo_f) and dU_j = min(0, D_f) (unknown_f - clean unknown_f).  Summation order:
 *     thread t of 256 adds the differences of the features t, t + 256, .. of each branch's rectangle of reached features (conv1,
 *     conv2, conv3, out4; within a rectangle the channel runs fastest, then the column, then the row), the 64 lanes of a wave
 *     are added by a butterfly (distance 32, 16, .., 1), the four waves in order; then
 *       lb_j = c0_c - c0_j + ((S_j + dS_j) + (U_j + dU_j)),   worst = the first j that attains the minimum;
 *     a position that is open with 1 <= k <= enum_bits unknown stem bits goes through stage 2 in its workgroup (the code of
 *     ttnet_certify_u8's stage 2, started from S_j + dS_j).
 * Row and column 31 lie in no field: a position that touches only them has the clean planes and sums.
 *
 * map_dev receives [n][P] records of 16 bytes (8-byte aligned): { double lb; int32 worst; uint16 stage; uint16 unknown_stem; },
 * lb, worst, stage (0, 1, 2) and unknown_stem as in ttnet_certify_u8's record.  rows_dev receives n records of 32 bytes:
 *   { double lb_min; int32 pos_min; int32 worst; int32 certified; int32 interval; int32 enumeration; int32 positions; }
 * lb_min = the smallest lb over the positions, pos_min the first position that attains it, worst that position's; interval and
 * enumeration count the positions of stage 1 and 2, certified is their sum, positions = P.  An image is patch-certified when
 * certified == positions; only stride 1 makes that a statement about every placement.  A class outside 0..9: stage 0, worst -1
 * and lb = -inf at every position, not an error.
 *
 * Float64 in a fixed order, no float atomics, nothing read back; the same bytes on every run and whatever else the batch holds.
 * n * P workgroups are cut into launches (csrc/partition.h).  The lane's planes are ttnet_certify_u8's; 112 more bytes per image
 * of max_batch are allocated by the first call on a lane.  Errors: those of ttnet_certify_u8 (without eps), and patch_h, patch_w,
 * stride or amp outside their ranges or map_dev NULL or misaligned TTNET_E_INVALID. */
int ttnet_certify_patch_u8(ttnet_plan *plan, int lane, const uint8_t *x_nhwc_dev, int64_t n, const int32_t *classes_dev, int patch_h,
                           int patch_w, int stride, int amp, int enum_bits, double min_margin, void *rows_dev, void *map_dev,
                           void *stream);

/* Falsified PATCH robustness of TTNET_VALEXNET: for every position of ttnet_certify_patch_u8 (the same positions, stride and amp) a
 * search for a concrete uint8 fill of the patch, each byte inside [max(0, b - amp), min(255, b + amp)] of its clean byte b, on
 * which the image loses its class (csrc/attack.hip; DESIGN.md: falsified patch robustness).  The entry PREDICTS; a witness is a
 * witness only once ttnet_forward_u8 has judged it (ttnet_patch_paste_u8 builds the image, ttnet_attack_select_u8 with round = 0
 * and n_cand = 1 takes the margin), as for the L-infinity search.
 *   per image, once ("patch.base"): the clean pass of ttnet_certify_patch_u8;
 *   per (image, position), one workgroup of 256 threads ("patch.attack"), cut into launches as the sweep is (csrc/partition.h).
 * Predicted margin m_pred of a fill: with the fill pasted into the image, the lb_interval that ttnet_certify_box_u8 gives for the
 * degenerate box lo = hi = that image -- the same real number, computed as the sweep computes its bound: the pooled cells whose
 * field meets the patch again at radius 0 by stage 0's code, the features they reach, the differences dS_j, dU_j against the
 * clean feature planes in the sweep's summation order, lb_j = c0_c - c0_j + ((S_j + dS_j) + (U_j + dU_j)), worst = the first j
 * that attains the minimum.  A recomputed cell within the stem slack of zero is unknown and m_pred is then a lower bound of the
 * exact-arithmetic margin; otherwise it IS that margin.
 * Movable bits: the stem bits that the box of the position leaves unknown (what the sweep's stage 0 computes), fixed over the
 * rounds.  State: the current fill (initially the clean bytes), its stem planes, its m_cur and runner-up j_cur.  One round
 * (rounds in 1..4):
 *   gains, pushes  g_s for every movable bit on the current planes (a bit within the slack counts as 0) with D_f = A[f][c] -
 *                  A[f][j_cur], and wt_s for modes 0 and 1: the terms, their order and the flipped lookup of
 *                  ttnet_attack_propose_u8, the unflipped value read from the table too.
 *   scores         through Wsum in ttnet_attack_propose_u8's order (ch, then py, then px), for the bytes of the patch only; every
 *                  other byte scores 0 and never moves; M = max |score| over the patch, per mode.
 *   candidates     eight, index 4 mode + tau index.  tau in {0, 1/8, 1/4}: a byte with score != 0 and |score| > tau M takes the upper
 *                  (score > 0) or lower end of its box, every other byte keeps the current fill's value.  The two slots of tau =
 *                  1/2 (3 and 7) hold another proposal: the sign corner of mode 1 (upper end where the score is positive, lower end
 *                  where negative, the current byte where zero) with the bytes i for which H(position, round, 11 + slot, i) is set
 *                  at the opposite end; H = bit 16 of v after v = position * 0x9E3779B1 + (8 round + 11 + slot) * 0x85EBCA6B + i *
 *                  0xC2B2AE35, v ^= v >> 15, v *= 0x2C1B3C6D, v ^= v >> 12, v *= 0x297A2D39, v ^= v >> 15 in 32 bits; i = the byte's
 *                  index in the fill record.  In round 1 of a 1 x 1 patch the eight candidates are its eight corners instead:
 *                  candidate k gives channel ch the upper end if bit ch of k is set, else the lower end.
 *   selection      every candidate gets its m_pred (a candidate byte-equal to an earlier one of the round is not evaluated: it
 *                  cannot win); the smallest wins, ties go to the lowest index; it replaces the state only if strictly below m_cur.
 * The search stops after a round that leaves m_cur < -min_margin.  No search -- round 0, fill = the clean bytes, m_pred = the
 * clean value -- where the class is outside 0..9 (m_pred -inf, worst -1, unknown 0; not an error), where the clean m_pred is
 * already below -min_margin, and where the position has no movable bit (a position that touches only row or column 31 included).
 *
 * map_dev receives [n][P] records of 16 bytes (8-byte aligned): { double m_pred; int32 worst; uint16 round; uint16 unknown; },
 * round = the round that produced the kept fill, unknown = the cells of the kept fill's recomputed span that are within the slack
 * (round 0: of the clean planes); unknown == 0 means m_pred is exact.  fills_dev receives uint8 [n][P][192] (4-byte aligned): the
 * first 3 patch_h patch_w bytes hold the patch row-major (y, x, channel), the rest are zero.
 *
 * Float64 in a fixed order, no float atomics, nothing read back: the same bytes on every run, lane and batch composition.  A and
 * Wsum are built by the first call after a (re)load, as ttnet_attack_propose_u8 does; the lane's buffers are the sweep's,
 * allocated by the first call on a lane.  Errors: those of ttnet_certify_patch_u8 (without enum_bits and rows_dev), and rounds
 * outside 1..4 or fills_dev NULL or misaligned TTNET_E_INVALID; any other variant TTNET_E_UNSUPPORTED.  Nothing is launched in an
 * error case. */
int ttnet_attack_patch_u8(ttnet_plan *plan, int lane, const uint8_t *x_nhwc_dev, int64_t n, const int32_t *classes_dev,
                          int patch_h, int patch_w, int stride, int amp, int rounds, double min_margin,
                          void *map_dev, uint8_t *fills_dev, void *stream);

/* Witnesses as images: out_nhwc_dev[k] (uint8 [m][32][32][3]) = image tasks_dev[k] / P of x_nhwc_dev ([n][32][32][3]) with the fill of
 * task tasks_dev[k] = image * P + position (fills_dev: [n][P][192] as ttnet_attack_patch_u8 writes it) pasted at its position; a task
 * outside [0, n P) leaves out[k] all zero.  One launch on `stream` ("patch.paste").  Errors: patch_h, patch_w or stride outside
 * their ranges, m < 1, n outside [1, max_batch], a NULL or misaligned pointer (4 bytes for images and fills, 8 for tasks)
 * TTNET_E_INVALID; any other variant TTNET_E_UNSUPPORTED; before finalize TTNET_E_STATE. */
int ttnet_patch_paste_u8(ttnet_plan *plan, const uint8_t *x_nhwc_dev, int64_t n, int patch_h, int patch_w, int stride,
                         const uint8_t *fills_dev, const int64_t *tasks_dev, int64_t m, uint8_t *out_nhwc_dev, void *stream);

/* Falsified L-infinity robustness of TTNET_VALEXNET on the device: a search for uint8 witnesses (csrc/attack.hip; DESIGN.md:
 * falsified robustness).  ttnet_certify_u8 bounds the robust accuracy from below; an image is FALSIFIED when a concrete uint8
 * image inside the integer box [max(0, b - e), min(255, b + e)] (e = eps_levels byte levels; the box lies inside the real box
 * of the certificate at eps >= e) is held on which ttnet_forward_u8 does not give the class.  The forward itself checks a
 * witness, so falsified is never wrong; the search decides nothing, an image it leaves open stays open.  The caller drives the
 * rounds with the two entries below and ttnet_forward_u8:
 *
 *   round 0   forward of x0 (n images), then ttnet_attack_select_u8 with cand = x0, n_cand = 1, round = 0: initialises x_cur = x0,
 *             the records, the runner-ups and the active flags.
 *   round r   forward of x_cur on `lane` (n images; in round 1 the forward of x0 still stands), ttnet_attack_propose_u8 on that
 *             lane, forwards of the 8 n candidates (any lane, chunks of at most max_batch) into one [8 n][10] float32 buffer,
 *             ttnet_attack_select_u8 with n_cand = 8.
 *
 * The float32 fields of a record are those of the forwards that ran: the last bits of a logit depend on the number of images in
 * a forward (lin1's split-K count; the same up to 256 images), so a caller who wants records that do not depend on the batch an
 * image came in keeps every forward of a search at or below 256 images, as scale_imagenet_amd/attack.py does.
 *
 * ttnet_attack_propose_u8 reads the stage buffers of the forward last issued on `lane` ("features.4" stem bits, "features.5"
 * feature bits), which must have been the forward of xcur_dev.  Per image with active_dev[i] != 0, class c = classes_dev[i] and
 * runner-up j = worst_dev[i] (both in 0..9 and different; else the image counts as not active), with D_f = A[f][c] - A[f][j]
 * (float64, A of ttnet_certify_u8):
 *   gains      for every UNKNOWN stem bit s = (ch, py, px) -- the planes lo and hi of stem_planes_dev differ there; uint64
 *              [2][n][64][10], lo then hi, the first two parts of ttnet_certify_u8's planes_dev --
 *                g_s = sum D_f (y_f(bits with s flipped) - y_f(bits))
 *              over the at most 21 features whose windows hold s (6 of conv1, 6 of conv2, 8 of conv3, 1 of out4), in that branch
 *              order and raster order of the output position (output channel for conv3) inside a branch; every term is +D_f,
 *              -D_f or nothing; the flipped lookup is the table read at index ^ mask; paddings are known zeros.  g_s = 0 for
 *              every other bit.  gains_dev: NULL, or [n][6400] float64 that receives g ([64][10][10]; zeros for an image that is
 *              not active).
 *   push       wt_s = -g_s (bit_s == 0 ? +1 : -1) sign(bn_scale[ch]) (sign(0) = +1; the folded scale of the stem BatchNorm):
 *              mode 0 for the unknown bits with g_s < 0 and zero elsewhere, mode 1 for every unknown bit.
 *   score      score[y][x][k] = sum_s wt_s Wsum[ch_s][k][y - 3 py_s + 1][x - 3 px_s + 1] over the bits whose 5 x 5 field holds the
 *              pixel (at most 2 x 2 pooled cells x 64 channels), ch ascending, then py, then px, each product and each sum
 *              rounded on its own.  Wsum[ch][k][5][5] = the nine 3 x 3 stem kernels of (ch, k) shifted to the nine positions
 *              (dy, dx ascending) of the MaxPool(3) window and summed, float64 from the float32 weights.  Row and column 31 lie
 *              in no field and never change.
 *   candidates cand_dev uint8 [n][8][32][32][3], index 4 mode + tau index, tau in {0, 1/8, 1/4, 1/2}: with M = max |score| of the
 *              image and mode a byte is selected when score != 0 and |score| > tau M; a selected byte takes the upper end of the
 *              box of x0_dev's byte when score > 0, the lower end when score < 0; every other byte keeps xcur_dev's.  An image
 *              that is not active gets eight copies of its xcur_dev image.
 *
 * ttnet_attack_select_u8 takes logits_dev float32 [n * n_cand][10] (image-major, as cand_dev [n][n_cand][32][32][3]).  Per active
 * image and candidate m = l[c] - max_{j != c} l[j] in float32 (runner-up: the first of equal maxima); a candidate with a NaN logit
 * is skipped; the smallest m wins, ties go to the lowest index.  If it is below the image's best so far the candidate is copied
 * to xcur_dev, worst_dev[i] becomes its runner-up and best, worst, round, changed (bytes of x_cur that differ from x0) and linf
 * (largest |x_cur - x0|) are recorded; the image is falsified and active_dev[i] becomes 0 when m < -min_margin.  round = 0
 * initialises first: x_cur = x0, worst -1, active = (class in 0..9), record { margin0 NaN, best +inf, the rest 0 }; margin0 is
 * candidate 0's m; a falsified image then gets status 1 (wrong at x0), in later rounds 2.  A class outside 0..9 is NOT an error:
 * that image gets margin0 = best = -inf, worst -1, status 0 and is never active.  tried counts the candidates compared.
 * rows_dev holds n records of 32 bytes (8-byte aligned):
 *   { float margin0; float best; int32 worst; int32 status; int32 round; int32 changed; int32 linf; int32 tried; }
 * status: 0 open, 1 wrong at x0, 2 falsified by the search.  With min_margin at least the logit tolerance of ttnet_forward_u8 a
 * falsified image is not robust for the exact-arithmetic network either, the one ttnet_certify_u8 speaks of.
 *
 * Both calls launch on `stream` and return; no read-back and no synchronisation, except that the first propose after a (re)load
 * builds A and Wsum as ttnet_certify_u8 does (and synchronises once).  Fixed summation order, integer work and maxima: the same
 * input gives the same bytes.  With profiling on, ttnet_plan_last_timings reports the step "attack.propose" / "attack.select" of
 * the call.  Errors: eps_levels outside 0..64, n_cand outside 1..8, round < 0, min_margin NaN, a bad lane, n outside
 * [1, max_batch], a NULL or misaligned pointer (4 bytes for images, logits, classes, worst_dev, active_dev and candidates, 8 for
 * records, planes and gains; gains_dev alone may be NULL), xcur_dev equal to cand_dev or x0_dev in select TTNET_E_INVALID; any
 * variant other than TTNET_VALEXNET TTNET_E_UNSUPPORTED; before finalize, or propose when the last forward on `lane` ran another
 * n, TTNET_E_STATE.  Nothing is launched in an error case. */
int ttnet_attack_propose_u8(ttnet_plan *plan, int lane, const uint8_t *x0_dev, const uint8_t *xcur_dev, int64_t n,
                            const int32_t *classes_dev, const int32_t *worst_dev, const uint64_t *stem_planes_dev, int eps_levels,
                            const int32_t *active_dev, uint8_t *cand_dev, double *gains_dev, void *stream);
int ttnet_attack_select_u8(ttnet_plan *plan, const uint8_t *cand_dev, const float *logits_dev, int64_t n, int n_cand,
                           const int32_t *classes_dev, double min_margin, const uint8_t *x0_dev, uint8_t *xcur_dev, void *rows_dev,
                           int32_t *worst_dev, int32_t *active_dev, int round, void *stream);

/* Integer facts about the plan: "fcsize", "n_classes", "n_state_tensors", "max_batch",
 * "near_ties:<block_tt name>" (entries with |pre-activation| < 1e-5 found while building
 * that table), "table_bytes", "usage_bytes", "care_bytes", "care_blocks", "last_n:<lane>" (images of the
 * forward last issued on that lane), "workspace_bytes", "graph_replays" (forwards replayed from a
 * captured hipGraph so far), "graphs_enabled" (0: ttnet_last_error() then says why), "graph_captures",
 * "graph_drops", "graphs_cached", "lanes", "range_overflow" (synchronises; 1 if a forward since the last
 * query left the fp16 x 2 range, and clears the flag), "gate_path" (which kernels evaluate the blocks, fixed at
 * finalize: 0 the two launches per block of TT-small, also kept by TTNET_GATE_UNFUSED=1; 1 one fused launch per
 * block; 2 x-small; 3 full; 4 vAlexnet), "gate_grid:<block index>" (paths 0 and 1: workgroups of that block's
 * first launch at the batch size of the forward last issued on the lane used last). */
int ttnet_plan_query(ttnet_plan *plan, const char *what, int64_t *out);

/* How the launchers cut a batch into slices, rounds, runs and chunks (csrc/partition.h), read out by name.  Stateless:
 * no plan, no device, no HIP call; it answers on a machine without a GPU.  `what` names a quantity, `args` are its n_args
 * integer arguments, and the values are written to out[0 .. return value).  Keys, arguments -> values:
 *   "slices_for" (n, units, target) -> slices          "slice" (sl, n, slices) -> n0, n1
 *   "fused.const" () -> threads, table buffer bytes, round bytes, workgroups at most      "fused.round" (HO) -> images per round
 *   "fused.launch" (C, HO, n) -> grid, slices, R, placement (0 plain, 1 quad, 2 pairs of 8)    "fused.owner" (b, C, n) -> strand, slice
 *   "two_launch.const" () -> depthwise, conv3, convf workgroup targets
 *   "two_launch.stage1" (C, n) -> grid, depthwise units, their slices, conv3 units, their slices    "two_launch.pf" (C, n) -> units, slices
 *   "flat.xs_branches" (C, Ho), "flat.xs_pf" (C, Ho), "flat.xs_last" (C, Ho, Wo), "flat.va_dw" (), "flat.va_c3" (), "flat.va_feat" ()
 *       -> tasks per image, threads per workgroup
 *   "full.const" () -> depthwise rows per chunk, its grid cap, the grid of its list pass, 1x1 wave tasks per chunk, its grid cap,
 *       the grid cap of its list pass, listed pixels per wave task, the share of the main pass's tasks that pass is sized for
 *   "full.row_bundle" (H, W) -> rows per wave task, wave tasks per image      "full.dw" (n, C, ho) -> chunks, chunks at most
 *   "full.pw" (n, groups, H, W) -> wave tasks, chunks, chunks at most, chunks of the list pass
 *   "full.fix" (n, groups, H, W, listed) -> wave tasks of a group's list, chunks      "full.fix_entries" (groups, H, W) -> list entries per image
 *   "stem.const" () -> items per image, stage buffers, workgroups on the whole chip, on half of it
 *   "stem.workgroups" (lanes, u8, full variant) -> workgroups asked for       "stem.grid" (n, G) -> workgroups launched
 *   "stem.run" (bid, n, G) -> first item, items                               "stem.continues" (first item, j) -> 0 / 1
 *   "patch.sweep" (n, patch_h, patch_w, stride) -> positions down, across, launches of ttnet_certify_patch_u8's sweep, workgroups
 *       of the first launch, of the last, at most      "patch.attack" (the same) -> the same for ttnet_attack_patch_u8's search
 * Returns the number of values written.  An unknown key, a wrong n_args, out_cap below the key's value count, n < 1, C not a
 * multiple of 8 (16 for "two_launch.stage1") or any argument outside its range: TTNET_E_INVALID with the reason in
 * ttnet_last_error(), and nothing is written. */
int ttnet_launch_partition(const char *what, const int64_t *args, int n_args, int64_t *out, int out_cap);

/* Device time of the kernels of the last forward, measured with HIP events on the stream
 * the kernels were launched on (enable with ttnet_plan_set_profiling).  names/ms are
 * arrays of capacity `cap`; returns the number of entries.  Synchronises. */
int ttnet_plan_set_profiling(ttnet_plan *plan, int enabled);
int ttnet_plan_last_timings(ttnet_plan *plan, const char **names, float *ms, int cap);

void ttnet_plan_destroy(ttnet_plan *plan);

/* Multi-GPU: the path shards by image (eval BatchNorm uses running statistics; nothing
 * crosses samples).  The only exchange is the gather of logits that
 * torch.nn.DataParallel.gather performs on GPU 0 in the reference (main.py:192).  One
 * process per GPU; `unique_id` is the 128-byte ncclUniqueId from ttnet_comm_unique_id on
 * rank 0, distributed by the caller (e.g. through its torch.distributed store). */
int ttnet_comm_unique_id(void *id128);
int ttnet_comm_create(const void *id128, int rank, int world, int device, ttnet_comm **out);
int ttnet_allgather_logits(ttnet_comm *comm, const float *local_dev, int64_t n_local, int64_t n_classes,
                           float *all_dev, void *stream);
void ttnet_comm_destroy(ttnet_comm *comm);

const char *ttnet_last_error(void);
const char *ttnet_version(void);

#ifdef __cplusplus
}
#endif
#endif /* TTNET_H */
