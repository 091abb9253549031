/*
 * igan_hip.h -- C ABI of libigan_hip.so: the MI355X (gfx950) kernels behind the
 * InclusiveGAN G/D forward+backward hot path.
 *
 * This is the drop-in boundary for the reference's two native plugin mechanisms:
 *   (1) the TF custom ops loaded by dnnlib/tflib/custom_ops.py:87-167
 *       (UpFirDn2D  -> dnnlib/tflib/ops/upfirdn_2d.cu:310-324,
 *        FusedBiasAct -> dnnlib/tflib/ops/fused_bias_act.cu:174-186), and
 *   (2) the convolution / matmul / reduction / optimizer arithmetic the reference
 *       obtains from TensorFlow+cuDNN (networks_stylegan2.py:46,60,120,
 *       upfirdn_2d.py:291,332, optimizer.py:318-332) and the nearest-neighbour
 *       search it obtains from dci_code (dci.h:76-89).
 *
 * Conventions (same contract as the reference ops):
 *   - plain pointers and sizes only; no torch / TF types;
 *   - the CALLER owns every buffer (inputs, outputs, workspaces); nothing is
 *     allocated, retained or freed by the library;
 *   - every entry point enqueues work on the given hipStream_t and returns
 *     without synchronising (graph-capturable, re-entrant);
 *   - return value 0 == IGAN_OK; on failure a thread-local message is available
 *     from igan_last_error() (invalid arguments mirror the reference's
 *     OP_REQUIRES checks, e.g. upfirdn_2d.cu:228-229,241-244,252,256,266);
 *   - element counts are limited to int32 like the reference (upfirdn_2d.cu:243); operands the
 *     conv / 1-NN kernels read through buffer descriptors are limited to 2 GiB each.
 *   - all activation tensors are fp32, channel-minor ("NHWC"): [N, H, W, C].
 */
#ifndef IGAN_HIP_H
#define IGAN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever a struct layout, a signature or the set of exports changes (2: fused conv epilogue fields, fp64 nearest-neighbour state;
 * 5 / 6: piece images and their sizes; 7: igan_conv_piece_form, igan_debug_f16_window; 8: the two-piece fp16 form scales every tensor per
 * pixel (forward / data gradient) or per channel (weight gradient) and writes its own images -- caller-written images (igan_to_pieces, x_pieces,
 * dy_pieces) belong to the bf16-piece form only; igan_conv2d_params gains x_colmax, igan_conv2d_wgrad_params x_colmax / dy_colmax at their ends;
 * 9: igan_conv2d_params gains w_pieces / w_pieces_bytes -- a caller-kept FILTER image for weights that never change (igan_filter_image_bytes, igan_filter_image);
 * 10: igan_knn_radius_update, igan_manifold_member_update; added under 10 without a bump, exports only: igan_ppl_endpoints, igan_ppl_crop_prep,
 * igan_linear_svc_workspace_bytes, igan_linear_svc_grad, igan_linear_svc_hv, igan_linear_svc_linesearch, igan_linear_svc_predict,
 * igan_images_to_uint8, igan_images_from_uint8, igan_dense_small2_grouped, igan_dense_small_wgrad2_grouped, igan_rows_group_sum,
 * igan_scale_add, igan_kmeans_workspace_bytes, igan_kmeans_step, igan_moments_workspace_bytes, igan_moments_update, igan_moments_finalize,
 * igan_moments_merge, igan_class_hist_update, igan_prob_stats_update, igan_nnk_update, igan_softmax_xent_fwd, igan_softmax_xent_bwd,
 * igan_xent_stats_update, igan_sigmoid_xent_fwd, igan_sigmoid_xent_bwd, igan_sigmoid_xent_stats_update, igan_binary_probs,
 * igan_filter_images_grouped (with struct igan_filter_image_desc, igan_struct_size id 9), igan_debug_filter_image_launches,
 * igan_manifold_member_nn1_update, igan_ball_count_update, igan_poly3_kernel_sums_workspace_bytes, igan_poly3_kernel_sums);
 * likewise, for the differentiable augmentation of D's inputs: igan_diffaugment_workspace_bytes, igan_diffaugment_fwd, igan_diffaugment_bwd. */
#define IGAN_ABI_VERSION 10

typedef void* igan_stream_t; /* hipStream_t */

enum igan_status {
    IGAN_OK = 0,
    IGAN_ERR_INVALID_ARGUMENT = 1, /* reference: errors::InvalidArgument */
    IGAN_ERR_HIP = 2,              /* reference: errors::Internal(cudaGetErrorName) */
    IGAN_ERR_UNSUPPORTED = 3
};

int igan_abi_version(void);
/* sizeof() of the parameter structs as this library was compiled, by id: 0 upfirdn2d, 1 fused_bias_act, 2 conv2d,
 * 3 conv2d_wgrad, 4 dense, 5 dense_wgrad, 6 taps, 7 dense2, 8 dense_wgrad2, 9 filter_image_desc; 0 for an unknown id.  A binding checks these against its own
 * struct declarations at load time, so that a stale library can never be driven with a newer struct (or vice versa). */
size_t igan_struct_size(int which);
const char* igan_last_error(void);

/* ------------------------------------------------------------------------
 * upfirdn2d: pad -> zero-insert upsample -> FIR -> decimate.
 * Replaces UpFirDn2DOp<T>::Compute + UpFirDn2DKernel_{small,large}
 * (dnnlib/tflib/ops/upfirdn_2d.cu:33-59,64-207,232-307).
 *   y[m,oy,ox,c] = sum_{ky,kx} xup_pad[m, oy*downy+ky, ox*downx+kx, c] * k[kH-1-ky, kW-1-kx]
 * outW/outH are derived exactly as upfirdn_2d.cu:254-255 and must match.
 * `k` is a HOST pointer (<= 64 taps; the reference wrapper always builds the
 * filter from a NumPy constant, upfirdn_2d.py:123-124); it is copied into the
 * kernel arguments, so the call stays graph-capturable.
 */
typedef struct igan_upfirdn2d_params {
    const float* x; /* [majorDim, inH, inW, minorDim] device */
    const float* k; /* [kernelH, kernelW] HOST */
    float* y;       /* [majorDim, outH, outW, minorDim] device */
    int upx, upy, downx, downy;
    int padx0, padx1, pady0, pady1;
    int majorDim, inH, inW, minorDim;
    int kernelH, kernelW;
    int outH, outW;
} igan_upfirdn2d_params;

int igan_upfirdn2d(igan_stream_t stream, const igan_upfirdn2d_params* p);
/* The half instantiation the reference registers next to float (REGISTER_KERNEL_BUILDER ... Eigen::half, upfirdn_2d.cu:323-324):
 * `x` and `y` hold IEEE binary16 values behind the float-typed fields (cast the pointers); `k` stays a host float array and is
 * rounded to half like the reference's `k: T` input; loads widen to float, the accumulation is float, the store rounds to half
 * (upfirdn_2d.cu:101,114).  General kernel only (no configuration of the training path runs in half). */
int igan_upfirdn2d_f16(igan_stream_t stream, const igan_upfirdn2d_params* p);
/* The same with the synthesis layer's epilogue fused into the store (layers whose FIR sits between the up-convolution and the
 * bias, networks_stylegan2.py:349-357 with up=True):  y = act(upfirdn(x) + noise[m, oy, ox] * strength[0] + bias[c]) * gain,
 * act in {1 linear, 2 relu, 3 lrelu} as igan_bias_act_noise_*; noise [majorDim or 1 (noise_bcast), outH, outW] or NULL with
 * strength.  Offered on the FIR fast path only (up = down = 1, taps <= 4x4, minorDim % 4 == 0); IGAN_ERR_UNSUPPORTED otherwise. */
int igan_upfirdn2d_ban(igan_stream_t stream, const igan_upfirdn2d_params* p, const float* noise, const float* strength,
                       int noise_bcast, const float* bias, int act, float alpha, float gain);

/* ------------------------------------------------------------------------
 * fused_bias_act: y = act(x + b[(i / stepB) % sizeB]) * gain  (grad == 0) and its
 * first / second derivative forms (grad == 1, 2) selected by act*10+grad.
 * Replaces FusedBiasActOp<T>::Compute + FusedBiasActKernel
 * (dnnlib/tflib/ops/fused_bias_act.cu:22-40,42-116,139-171).
 * act index follows fused_bias_act.py:20-30 (1 linear, 2 relu, 3 lrelu, 4 tanh,
 * 5 sigmoid, 6 elu, 7 selu, 8 softplus, 9 swish).
 */
typedef struct igan_fused_bias_act_params {
    const float* x;   /* [sizeX] */
    const float* b;   /* [sizeB] or NULL */
    const float* ref; /* [sizeX] or NULL (required iff grad != 0) */
    float* y;         /* [sizeX] */
    int grad;
    int act;
    float alpha;
    float gain;
    int sizeX;
    int sizeB;
    int stepB;
} igan_fused_bias_act_params;

int igan_fused_bias_act(igan_stream_t stream, const igan_fused_bias_act_params* p);
/* The half instantiation (fused_bias_act.cu:185-186): x / b / ref / y hold IEEE binary16 values behind the float-typed fields;
 * every element is widened to float, evaluated with the same table, and rounded on store (fused_bias_act.cu:56-61,113). */
int igan_fused_bias_act_f16(igan_stream_t stream, const igan_fused_bias_act_params* p);

/* Bias gradient: db[c] = sum over all i with (i / stepB) % sizeB == c of dx[i].
 * Replaces the TF reduce_sum pair of fused_bias_act.py:137-146.
 * Deterministic (fixed reduction order). `partial` is a caller-owned workspace of
 * igan_bias_grad_workspace_floats(sizeX, sizeB, stepB) floats. */
size_t igan_bias_grad_workspace_floats(int sizeX, int sizeB, int stepB);
int igan_bias_grad(igan_stream_t stream, const float* dx, float* db, float* partial,
                   int sizeX, int sizeB, int stepB);

/* Fused synthesis-layer epilogue (training/networks_stylegan2.py:351-357) on channel-minor data
 * x[rows = N*H*W][C], C % 4 == 0:
 *     y = act(x + noise[row] * (*strength) + b[c]) * gain          act in {1 linear, 2 relu, 3 lrelu}
 * noise/strength NULL -> plain apply_bias_act (networks_stylegan2.py:66-68).  The backward produces, in
 * ONE pass over (dy, y):  dx = dy * gain * act'(y)   (FusedBiasAct grad=1 with ref = y),
 *     db[c] = sum_rows dx   (fused_bias_act.py:137-146),   *dstrength = sum_rows noise[row] * sum_c dx.
 * db / dstrength may be NULL when not wanted.  Deterministic; `workspace` holds
 * igan_bias_act_noise_workspace_floats(rows, C) floats. */
size_t igan_bias_act_noise_workspace_floats(int rows, int C);
int igan_bias_act_noise_fwd(igan_stream_t stream, const float* x, const float* noise, const float* strength,
                            const float* b, float* y, int rows, int C, int act, float alpha, float gain);
int igan_bias_act_noise_bwd(igan_stream_t stream, const float* dy, const float* y, const float* noise,
                            float* dx, float* db, float* dstrength, float* workspace,
                            int rows, int C, int act, float alpha, float gain);

/* The same backward when the epilogue was fused into a modulated convolution (igan_conv2d with act / noise / out_scale:
 * y = act(d[n,c] * z + noise * strength + b) * gain, z never stored): additionally
 *     dd[n][c] = sum_{pixels of n} dx * z,      z = (pre - b[c] - noise * strength) / d[n][c],
 * the demodulation gradient of modulated_conv2d_layer (networks_stylegan2.py:105-107,126), with the pre-activation value
 * recovered from y (act 1 linear or 3 lrelu only).  y, dy, dx: [N, HW, C]; dscale = d [N, C]; noise [N or 1, HW] with
 * noise_bcast; workspace of igan_bias_act_noise_dd_workspace_floats(N, HW, C) floats.  One pass + one small reduce. */
size_t igan_bias_act_noise_dd_workspace_floats(int N, int HW, int C);
int igan_bias_act_noise_bwd_dd(igan_stream_t stream, const float* dy, const float* y, const float* noise, const float* strength,
                               const float* b, const float* dscale, float* dx, float* db, float* dstrength, float* dd,
                               float* workspace, int noise_bcast, int N, int HW, int C, int act, float alpha, float gain);

/* ------------------------------------------------------------------------
 * conv2d (implicit GEMM on the matrix cores, fp32 sums).  Three arithmetic forms, chosen once per process by IGAN_CONV_PLANES
 * (igan_conv_piece_form() tells which): 0 = every convolution on the fp32 matrix instruction (exact fp32 FMA chain); 1 = the large 3x3 layers from
 * three bf16 pieces per operand (all 24 significand bits, six products); 2 (default) = the large 3x3 layers from two fp16 pieces per operand
 * (<= 1 ulp of the fp32 operand, three products) under power-of-two scales that follow every axis a matrix-instruction chain does not sum over:
 * one per pixel of x in_scale and one per output channel of the filter in the forward / data-gradient kernel, one per channel of each operand in
 * the weight gradient.  Small, 1x1 and thin layers always run on the fp32 instruction.
 * One entry point covers what the reference gets from tf.nn.conv2d (SAME stride 1,
 * networks_stylegan2.py:60,120; VALID stride 2, upfirdn_2d.py:332),
 * tf.nn.conv2d_transpose (VALID stride 2, upfirdn_2d.py:291), tf.matmul
 * (networks_stylegan2.py:46, as a 1x1 conv on [N,1,1,C]) and their input
 * gradients:
 *
 *   y[n,oy,ox,co] = out_scale[n,co] * sum_{ky,kx,ci}
 *        xup[n, oy*stride + ky - pad_y, ox*stride + kx - pad_x, ci] * in_scale[n,ci] * W(ky,kx,ci,co)
 *   xup[n,v,u,ci] = x[n, v/up, u/up, ci] if v%up==0 && u%up==0 && in range else 0
 *
 * (cross-correlation, like tf.nn.conv2d).  w_transposed == 0: W(ky,kx,ci,co) =
 * w[ky][kx][ci][co] (HWIO, networks_stylegan2.py:23).  w_transposed == 1: the
 * buffer is the FORWARD layer's HWIO weight [KH][KW][Cout][Cin] and
 * W(ky,kx,ci,co) = w[KH-1-ky][KW-1-kx][co][ci] (spatial flip + channel swap) --
 * i.e. the data-gradient of a forward conv with (stride,up,pad) is this same entry
 * point called with (stride'=up, up'=stride, pad'=K-1-pad, w_transposed=1).
 * At most one of stride, up may exceed 1.  in_scale / out_scale (optional)
 * implement StyleGAN2 modulation / demodulation in the non-fused form of
 * networks_stylegan2.py:112,126.
 *
 * Tail slicing: the output is a list of tiles dealt to the CUs; when the list does not fill a whole number
 * of rounds, the last `sliced_tiles` tiles are cut into `splits` slices along the reduction axis (taps x Cin)
 * so that the last round occupies every CU.  Their partial tiles go to `workspace` (tile-compact,
 * sliced_tiles * splits tiles) and a fix-up kernel sums them in fixed order (bit-reproducible).
 * igan_conv2d_plan() chooses `splits`, `sliced_tiles` and the workspace size for a shape; pass them back.
 */
typedef struct igan_conv2d_params {
    const float* x;         /* [N, H, W, Cin] */
    const float* w;         /* see above */
    float* y;               /* [N, OH, OW, Cout] */
    const float* in_scale;  /* [N, Cin] or NULL */
    const float* out_scale; /* [N, Cout] or NULL */
    float* workspace;       /* igan_conv2d_plan()'s workspace_floats floats, 16-byte aligned; NULL iff the plan asked for none.  It
                             * holds the partial tiles of the sliced tail (splits > 1) and, for the shapes the library runs in a
                             * piece form (forms 1 and 2 above), the piece images of x and of the filter behind them (with their
                             * scales in form 2); a launch that gets no room for the images runs the fp32 kernel */
    size_t workspace_floats;
    int N, H, W, Cin;
    int OH, OW, Cout;
    int KH, KW;
    int stride, up;
    int pad_y, pad_x;
    int w_transposed;
    int splits;             /* reduction slices of each sliced tile (from igan_conv2d_plan; 1 = none) */
    int sliced_tiles;       /* how many trailing tiles of the tile list are sliced (from igan_conv2d_plan) */
    float alpha;            /* y is multiplied by alpha (the layers' runtime weight scale, networks_stylegan2.py:30-36,
                             * rides here instead of in a separate w * coef pass); 1.0f for a plain convolution */
    const float* bias;      /* fused epilogue (act != 0): y = act(y + bias[co]) * act_gain, the apply_bias_act that follows the
                             * convolution (networks_stylegan2.py:66-68); bias may be NULL */
    int act;                /* 0 = no epilogue; 1 linear, 2 relu, 3 lrelu (as igan_bias_act_noise_*) */
    float act_alpha, act_gain;
    const float* noise;     /* fused epilogue of a synthesis layer (networks_stylegan2.py:351-357): with act != 0,
                             * y = act(y + noise[n, oy, ox] * noise_strength[0] + bias[co]) * act_gain; NULL = no noise */
    const float* noise_strength; /* device scalar */
    int noise_bcast;        /* 1: noise is [1, OH, OW], shared by the batch (the layer's stored noise); 0: [N, OH, OW] */
    const void* x_pieces;   /* bf16-piece form (IGAN_CONV_PLANES=1) only: the piece image of x * in_scale, written by igan_to_pieces(),
                             * so that a caller who runs several convolutions on one tensor writes its image once.  NULL otherwise:
                             * the fp16 form rejects a non-NULL image (ABI v8: its images are scaled per pixel here and per channel in
                             * the weight gradient, so no image serves two calls), form 0 ignores it */
    size_t x_pieces_bytes;  /* its size, N * H * W * Cin * 6 (ABI v6): an image of any other size is rejected, never read */
    float* x_colmax;        /* ABI v8, fp16 form, optional OUTPUT (igan_colmax_floats(N, H * W, Cin) floats, 16-byte aligned; NULL = none): the per-channel maxima of
                             * |x * in_scale| -- a by-product of the row image this call writes of x (a pass of its own when the call takes another path), which a later
                             * igan_conv2d_wgrad() of the SAME tensor takes as x_colmax / dy_colmax instead of a pass of its own over it */
    const void* w_pieces;   /* ABI v9, piece forms, optional: the image of THIS call's filter (same w, KH, KW, Cin, Cout, w_transposed) written earlier by
                             * igan_filter_image() -- for weights that are constants of the run (the LPIPS network's: 36 filter images per generator step
                             * otherwise); the call then writes none.  NULL = the call images its filter itself.  Ignored by calls that run on the fp32 instruction */
    size_t w_pieces_bytes;  /* its size, igan_filter_image_bytes(KH, KW, Cin, Cout): an image of any other size is rejected, never read */
} igan_conv2d_params;

int igan_conv2d_plan(const igan_conv2d_params* p, int* splits, int* sliced_tiles, size_t* workspace_floats);
int igan_conv2d(igan_stream_t stream, const igan_conv2d_params* p);
/* Host-only: name of the kernel instantiation igan_conv2d() launches for these parameters (as reported
 * by rocprofv3, minus the anonymous-namespace prefix).  For profiling tools.
 * The thin-channel names carry the tap count only: "thin_out_kernel<1>" covers one and two channel blocks (thin_out_kernel<1, 1> and
 * <1, 2>, Cin = 512), and "thin_in_kernel<9>" also stands for the sliding-window kernel thin_in3x3_kernel<3> that takes a 3x3 filter
 * when Cin == 3, Cout <= 256 and OW >= 16. */
int igan_conv2d_kernel_name(const igan_conv2d_params* p, char* buf, int buflen);

/* Weight gradient of the op above (same geometry fields):
 *   dw[ky,kx,ci,co] = sum_{n,oy,ox} xup[n, oy*stride+ky-pad_y, ox*stride+kx-pad_x, ci]
 *                                   * in_scale[n,ci] * dy[n,oy,ox,co] * out_scale[n,co]
 * written in HWIO [KH][KW][Cin][Cout].  The pixel axis is always reduced through
 * the caller's workspace in fixed order (bit-reproducible);
 * igan_conv2d_wgrad_plan() returns the split count and workspace size (the partial filters of the pixel
 * slices; in the piece forms also the piece images of x and dy, as for igan_conv2d). */
typedef struct igan_conv2d_wgrad_params {
    const float* x;         /* [N, H, W, Cin] */
    const float* dy;        /* [N, OH, OW, Cout] */
    float* dw;              /* [KH, KW, Cin, Cout] */
    const float* in_scale;  /* [N, Cin] or NULL */
    const float* out_scale; /* [N, Cout] or NULL */
    float* workspace;
    size_t workspace_floats;
    int N, H, W, Cin;
    int OH, OW, Cout;
    int KH, KW;
    int stride, up;
    int pad_y, pad_x;
    int splits;
    float alpha;            /* dw is multiplied by alpha (see igan_conv2d_params) */
    const void* x_pieces;   /* bf16-piece form (IGAN_CONV_PLANES=1) only: piece images of x * in_scale and dy * out_scale; NULL otherwise (as igan_conv2d_params) */
    const void* dy_pieces;
    size_t x_pieces_bytes;  /* N * H * W * Cin * 6 and N * OH * OW * Cout * 6 (ABI v6): checked before an image is read */
    size_t dy_pieces_bytes;
    const float* x_colmax;  /* ABI v8, fp16 form, optional INPUTS (NULL = none): the buffers an igan_conv2d() call on the same x * in_scale / dy * out_scale filled (x_colmax there); */
    const float* dy_colmax; /* the column image of that operand then skips its maxima pass.  Bit-identical results either way (a maximum does not depend on the order). */
} igan_conv2d_wgrad_params;

int igan_conv2d_wgrad_plan(const igan_conv2d_wgrad_params* p, int* splits, size_t* workspace_floats);
int igan_conv2d_wgrad(igan_stream_t stream, const igan_conv2d_wgrad_params* p);
/* Host-only (ABI v6): the kernel family igan_conv2d_wgrad() runs for these parameters ("conv_wgrad_kernel",
 * "conv_wgrad_planes_kernel", "thin_wgrad_kernel", "dense_small_wgrad_kernel").  For profiling tools. */
int igan_conv2d_wgrad_kernel_name(const igan_conv2d_wgrad_params* p, char* buf, int buflen);

/* ABI v6: the library's own answer to "will a layer with this filter take a piece form?" (the batch-independent part of the
 * rule: 3x3 taps, both channel counts >= 128 and whole 32s, a piece form switched on) and "is a tensor [N, HW, C] one igan_to_pieces() can
 * image for it?" (form 1 only: always 0 in forms 0 and 2) -- so that a host does not restate the rules.  Both return 0 / 1. */
int igan_conv_pieces_wanted(int KH, int KW, int Cin, int Cout);
int igan_pieces_image_ok(int N, int HW, int C);
/* ABI v7: which piece form this process runs (read once from IGAN_CONV_PLANES): 0 = none (every convolution on the fp32 matrix instruction),
 * 1 = three bf16 pieces / six products, 2 = two fp16 pieces (the default when the variable is unset): p0 = fp16(v S), p1 = fp16((v S - p0) 2^11)
 * with a power-of-two S per scale group (ABI v8: a pixel's channel vector / a filter's output channel in the forward and data-gradient kernel, a
 * channel's pixels in the weight gradient -- never a whole tensor), three products; the operand to 2^-23 (exactly in three cases of four) for every
 * element within 2^26 of the largest of its own group. */
int igan_conv_piece_form(void);
/* ABI v9: the filter image of a convolution call as a caller-kept buffer.  igan_filter_image_bytes: its size for a call with this filter geometry (Cin / Cout are the
 * CALL's: a data-gradient call has them swapped against its forward layer), 0 = this process / filter takes none (form 0; a 1x1 or thin filter; a channel count outside
 * the piece form).  igan_filter_image: writes it (16-byte aligned `out`; the same kernels igan_conv2d runs for its own image, so results are bit-identical). */
size_t igan_filter_image_bytes(int KH, int KW, int Cin, int Cout);
int igan_filter_image(igan_stream_t stream, const float* w, void* out, int KH, int KW, int Cin, int Cout, int w_transposed);
/* Grouped form (fp16 form only; IGAN_ERR_UNSUPPORTED under the bf16-piece form and with the piece forms off): the images of `count` (<= IGAN_FILTER_MAX_GROUPS)
 * filters in exactly TWO kernel launches, whatever `count` is -- the column maxima of all entries, then the images and 1 / S of all entries.  An entry is what one
 * igan_filter_image call takes, and its image is byte for byte what that call writes, so a convolution call may be handed it as w_pieces.  For weights that change
 * between the ops of a training loop but not inside one: every filter image an op needs, written at its top from the current weights.  Checked before any device
 * work (igan_last_error() names the entry): every entry has igan_filter_image_bytes() != 0, 16-byte aligned w / out, and no two `out` ranges overlap. */
#define IGAN_FILTER_MAX_GROUPS 48
typedef struct igan_filter_image_desc { const float* w; void* out; int KH, KW, Cin, Cout, w_transposed; } igan_filter_image_desc;
int igan_filter_images_grouped(igan_stream_t stream, const igan_filter_image_desc* groups, int count);
/* Diagnostic (host side, no device work): kernel launches issued for filter images so far -- by igan_conv2d for its own image, igan_filter_image and
 * igan_filter_images_grouped; reset != 0 zeroes the counter after reading it. */
int igan_debug_filter_image_launches(unsigned long long* out, int reset);
/* ABI v8: size in floats of an x_colmax / dy_colmax buffer for a tensor [N, HW, C]; 0 = none is taken (not the fp16 form, a channel count outside it, or fewer
 * pixels than any weight gradient that takes the column image has: N * HW below the piece form's row threshold). */
size_t igan_colmax_floats(int N, int HW, int C);
/* Diagnostic for form 2 (synchronises the device): non-zero elements imaged so far BELOW the exact window (|v S| < 2^-12: more than 2^26 below the
 * largest magnitude of the element's own scale group) and elements imaged in all; reset != 0 zeroes both counters. */
int igan_debug_f16_window(unsigned long long* below, unsigned long long* imaged, int reset);
/* ABI v8: the same counters by kind of image, out4 = {rows below, rows imaged, columns below, columns imaged}: a ROW image (forward / data gradient) scales a
 * pixel's channel vector, a COLUMN image (weight gradient) a channel's pixels -- there the group runs along the summed axis, where an element 2^26 below the
 * group's largest stands next to that largest element in every sum it enters. */
int igan_debug_f16_window_by_kind(unsigned long long* out4, int reset);

/* bf16-piece form (IGAN_CONV_PLANES=1) only -- IGAN_ERR_UNSUPPORTED in the other forms: the piece image of a channel-minor tensor
 * x [N, HW, C] (times scale [N, C] when given), `out` = N * HW * C * 6 bytes, 16-byte aligned, C % 16 == 0.  The convolution entry
 * points write the images they need themselves; a caller that feeds one tensor to several of them (dy to the data and the
 * weight gradient, x to the forward pass and the weight gradient) writes it once with this and passes it as x_pieces / dy_pieces. */
int igan_to_pieces(igan_stream_t stream, const float* x, const float* scale, void* out, int N, int HW, int C);

/* ------------------------------------------------------------------------
 * Small-batch dense layers with the StyleGAN2 style-path arithmetic folded in (M <= 64 rows; larger
 * batches go through igan_conv2d as 1x1 convolutions):
 *     y[m,n] = epi( alpha * sum_k pro(x)[m,k] * W(k,n) ),   W = w[k][n], or w[n][k] when w_transposed
 * prologue (on x, element-wise):   NONE; SQUARE x^2; DEMOD_GRAD pro_scale * x * x2^3
 * epilogue:  SCALE  v
 *            BIAS   v + bias_scale * bias[n] + add_const                 (style affine + 1, networks_stylegan2.py:99-101)
 *            RSQRT  rsqrt(v + eps)                                         (demodulation coefficients, :105-107)
 *            STYLE_GRAD  e1[m,n] + 2 * e2[m,n] * v, and, if colsum != NULL, colsum[n] = bias_scale * sum_m y[m,n]
 * so that, with q = s^2 . wsq and d = rsqrt(c^2 q + eps):
 *     s  = BIAS(x=w_lat, W=A)                       d  = RSQRT(SQUARE s, W=wsq, alpha=c^2)
 *     ds = STYLE_GRAD(DEMOD_GRAD(dd, d; pro_scale=-c^2/2), W=wsq^T, e1=ds_conv, e2=s)   [+ bias gradient]
 * Weight-gradient form:  dw[k,n] = alpha * sum_m pro_a(a)[m,k] * pro_b(b)[m,n]   (pro_a NONE|SQUARE,
 * pro_b NONE|DEMOD_GRAD with b2).  K % 4 == 0 (dense), N % 4 == 0 (weight gradient); x / x2 / b / b2 / dw
 * 16-byte aligned.  Deterministic. */
enum { IGAN_DENSE_PRO_NONE = 0, IGAN_DENSE_PRO_SQUARE = 1, IGAN_DENSE_PRO_DEMOD_GRAD = 2 };
enum { IGAN_DENSE_EPI_SCALE = 0, IGAN_DENSE_EPI_BIAS = 1, IGAN_DENSE_EPI_RSQRT = 2, IGAN_DENSE_EPI_STYLE_GRAD = 3 };
typedef struct igan_dense_params {
    const float* x;         /* [M, K], row stride ldx floats (ldx % 4 == 0) */
    const float* x2;        /* DEMOD_GRAD: [M, K] contiguous, else NULL */
    const float* w;         /* [K, N], or [N, K] when w_transposed */
    float* y;               /* [M, N], row stride ldy floats */
    const float* bias;      /* BIAS: [N] */
    const float* e1;        /* STYLE_GRAD: [M, N] contiguous or NULL (= 0) */
    const float* e2;        /* STYLE_GRAD: [M, N] contiguous */
    float* colsum;          /* STYLE_GRAD: [N] or NULL */
    int ldx, ldy;
    int M, K, N;
    int w_transposed;
    int prologue, epilogue;
    float alpha, pro_scale, bias_scale, add_const, eps;
} igan_dense_params;
int igan_dense_small(igan_stream_t stream, const igan_dense_params* p);

typedef struct igan_dense_wgrad_params {
    const float* a;         /* [M, K], row stride lda floats */
    const float* b;         /* [M, N] contiguous */
    const float* b2;        /* DEMOD_GRAD: [M, N] contiguous, else NULL */
    float* dw;              /* [K, N] */
    int lda;
    int M, K, N;
    int pro_a, pro_b;
    float alpha, pro_scale;
} igan_dense_wgrad_params;
int igan_dense_small_wgrad(igan_stream_t stream, const igan_dense_wgrad_params* p);

/* Grouped forms: `count` (<= IGAN_DENSE_MAX_GROUPS) independent problems in ONE launch -- the 18 style affines, the 12
 * demodulations, and each stage of their backward, of one generator pass.  The groups of a dense launch share
 * `w_transposed`; sizes may differ per group. */
#define IGAN_DENSE_MAX_GROUPS 24
#define IGAN_DENSE_MAX_ROWS 64
int igan_dense_small_grouped(igan_stream_t stream, const igan_dense_params* groups, int count);
int igan_dense_small_wgrad_grouped(igan_stream_t stream, const igan_dense_wgrad_params* groups, int count);

/* The style path differentiated twice (path-length regulariser, training/loss.py:60-66), closed: with e = -c^2/2 gd d^3,
 * m = e . wsq^T, sigma = gs + 2 s m, the latent gradient dy = c_a sigma . A^T is a differentiable op whose own backward is
 * written out (hip_ops.StyleGradAllFn).  What its lines need beyond igan_dense_params:
 *     prologue MUL          pro_scale * x * x2                                    (r = 2 v s)
 *     y2 != NULL            with the epilogues above: y2[m,n] = alpha * sum, the product itself beside its epilogue form
 *     epilogue DEMOD_GRAD2  y = -1/2 v e2^3,  y2 = 3/4 v e1 e2^5                  (gd_bar and q_bar from v = c^2 e_bar; e1 = gd, e2 = d)
 *     epilogue STYLE_GRAD2  y = 2 (e2 v + e1 e3)  [+ colsum as STYLE_GRAD]        (s_bar; e2 = s, e1 = v, e3 = m)
 * and a two-term weight-gradient form
 *     dw[k,n] = alpha * sum_m a[m,k] a2[m,k] pro_b(b)[m,n] + alpha2 * sum_m pro_c(c)[m,k] d[m,n]
 * (a2 NULL = 1; c NULL = no second term; pro_b NONE|DEMOD_GRAD with b2, pro_c NONE|SQUARE).  e3 / y2 / a2 / d are contiguous [M, N] / [M, K].
 * igan_struct_size ids 7 and 8. */
enum { IGAN_DENSE_PRO_MUL = 3 };
enum { IGAN_DENSE_EPI_DEMOD_GRAD2 = 4, IGAN_DENSE_EPI_STYLE_GRAD2 = 5 };
typedef struct igan_dense2_params {
    igan_dense_params p;
    const float* e3;
    float* y2;
} igan_dense2_params;
int igan_dense_small2_grouped(igan_stream_t stream, const igan_dense2_params* groups, int count);

typedef struct igan_dense_wgrad2_params {
    const float* a;         /* [M, K], row stride lda floats */
    const float* a2;        /* [M, K] contiguous or NULL */
    const float* b;         /* [M, N] contiguous */
    const float* b2;        /* DEMOD_GRAD: [M, N] contiguous, else NULL */
    const float* c;         /* [M, K], row stride ldc floats, or NULL */
    const float* d;         /* [M, N] contiguous (with c) */
    float* dw;              /* [K, N] */
    int lda, ldc;
    int M, K, N;
    int pro_b, pro_c;
    float alpha, pro_scale, alpha2;
} igan_dense_wgrad2_params;
int igan_dense_small_wgrad2_grouped(igan_stream_t stream, const igan_dense_wgrad2_params* groups, int count);

/* out[m, j, :] = sum over the groups l with slot[l] == j, in order, of src[l, m, :]  (zero where no group names j): the per-layer
 * latent gradients [count, M, D] of one synthesis pass gathered into the gradient of the latents [M, L, D].  `slot` is a HOST
 * pointer (count <= IGAN_DENSE_MAX_GROUPS entries), every entry in [0, L): a value outside is IGAN_ERR_INVALID_ARGUMENT, not a
 * group left out.  D % 4 == 0; deterministic. */
int igan_rows_group_sum(igan_stream_t stream, const float* src, const int* slot, int count, float* out, int M, int L, int D);

/* out[i] = sum_t w[t*n + i]^2  (sum over the filter taps of the squared weights: the [Cin,Cout] matrix of the
 * demodulation, :105) and out[t*n + i] = scale * w[t*n + i] * v[i] (its gradient back onto the filter). */
int igan_sumsq_taps(igan_stream_t stream, const float* w, float* out, int taps, int n);
int igan_bcast_mul_taps(igan_stream_t stream, const float* w, const float* v, float* out, int taps, int n, float scale);
typedef struct igan_taps_params {
    const float* w;         /* [taps, n] */
    const float* v;         /* bcast_mul: [n]; sumsq: unused (NULL) */
    float* out;             /* sumsq: [n]; bcast_mul: [taps, n] */
    int taps, n;
    float scale;            /* bcast_mul only */
} igan_taps_params;
int igan_sumsq_taps_grouped(igan_stream_t stream, const igan_taps_params* groups, int count);
int igan_bcast_mul_taps_grouped(igan_stream_t stream, const igan_taps_params* groups, int count);

/* Per-sample channel dot products of two channel-minor tensors a, b [N, HW, C] (C % 4 == 0):
 *     dot[n,c] = sum_hw a[n,hw,c] * b[n,hw,c];   if out != NULL: out[n,hw,c] = b[n,hw,c] * s[n,c]
 * (out may alias b; s may be NULL = 1).  These are the style / demodulation gradients of
 * modulated_conv2d_layer in its non-fused form (networks_stylegan2.py:112,126): ds = dot(x, g) with
 * dx = g * s, and dd = dot(dy, y) / d.  Deterministic; workspace of
 * igan_scale_dot_workspace_floats(N, HW, C) floats. */
size_t igan_scale_dot_workspace_floats(int N, int HW, int C);
int igan_scale_dot(igan_stream_t stream, const float* a, const float* b, const float* s, float* out,
                   float* dot, float* workspace, int N, int HW, int C);

/* out[n,hw,c] = a[n,hw,c] * alpha[n,c] + b[n,hw,c] * beta[n,c] on channel-minor tensors (C % 4 == 0): the element-wise lines of the
 * modulated convolution's second-order backward in one pass.  Either term may be absent (a or b NULL); alpha / beta NULL = 1;
 * out may alias a (every element is read before it is written, by the lane that writes it), not b. */
int igan_scale_add(igan_stream_t stream, const float* a, const float* alpha, const float* b, const float* beta, float* out,
                   int N, int HW, int C);

/* LPIPS per-layer distance (Zhang et al. 2018; role of lpips.get_output_for, training/loss.py:31,41) on raw
 * channel-minor VGG features fa, fb [N, HW, C], C in {64,128,256,512}, lin[C] >= 0:
 *     partial[n][j] = sum over block j's pixels of sum_c lin_c (fa_c/(|fa|+1e-10) - fb_c/(|fb|+1e-10))^2
 * (igan_lpips_layer_blocks(N, HW) partial sums per sample; caller adds them and divides by HW), and
 *     dfa = g[n] * d(distance sum)/d fa        (swap fa, fb for the other argument).  One pass each. */
int igan_lpips_layer_blocks(int N, int HW);
int igan_lpips_layer_fwd(igan_stream_t stream, const float* fa, const float* fb, const float* lin,
                         float* partial, int N, int HW, int C);
int igan_lpips_layer_bwd(igan_stream_t stream, const float* fa, const float* fb, const float* lin,
                         const float* g, float* dfa, int N, int HW, int C);
/* The same over a table of P sample pairs: row p compares sample ia[p] of fa with sample ib[p] of fb (NULL table =
 * identity) -- all four distances of the G loss (rec_1/real_1, rec_2/real_2, interp/real_2, interp/real_1, loss.py:31,41) in
 * one launch per layer.  Forward writes partial[p * partial_stride + j], j < blocks (caller picks blocks <= HW and lays the
 * layers' columns side by side so that one row sum finishes the distance).  Backward writes (accumulate = 0) or adds
 * (accumulate = 1) g[p] * d(distance sum)/d fa into sample ia[p] of dfa; two rows of one launch must not name the same
 * ia[p]. */
int igan_lpips_pairs_fwd(igan_stream_t stream, const float* fa, const float* fb, const float* lin, const int* ia,
                         const int* ib, float* partial, int partial_stride, int blocks, int P, int HW, int C);
int igan_lpips_pairs_bwd(igan_stream_t stream, const float* fa, const float* fb, const float* lin, const int* ia,
                         const int* ib, const float* g, float* dfa, int accumulate, int P, int HW, int C);

/* 2x2 max-pool between the VGG blocks of the LPIPS network (inside lpips.get_output_for, training/loss.py:31,41;
 * the network pickle is absent from the reference tree: restated) on channel-minor x [N, H, W, C] -> y [N, H/2, W/2, C],
 * and its gradient fused with the sum over the pooled map's two consumers (the map is also an LPIPS tap):
 *     dx = dskip + route(dy to the first maximum of each window in order (0,0) (0,1) (1,0) (1,1); NaN wins)
 * dskip may be NULL (= 0); dx may alias dskip.  H, W even, C % 4 == 0. */
int igan_maxpool2x2_fwd(igan_stream_t stream, const float* x, float* y, int N, int H, int W, int C);
int igan_maxpool2x2_bwd(igan_stream_t stream, const float* x, const float* dy, const float* dskip, float* dx,
                        int N, int H, int W, int C);

/* ------------------------------------------------------------------------
 * minibatch_stddev_layer statistics (networks_stylegan2.py:132-144), NHWC input
 * x[N, H, W, C], group size G (N % G == 0, M = N / G, num_new_features = 1):
 *   stat[m] = mean_{c,h,w} sqrt( mean_g (x[g*M+m] - mean_g x)^2 + 1e-8 )
 * fwd writes y[N, H, W, C+1] = concat(x, stat[n % M]); the statistic is reduced over position slices through
 * `workspace` (igan_mbstd_workspace_floats(N,H,W,C,G) floats, fixed order).
 * bwd takes dy[N,H,W,C+1] and returns dx[N,H,W,C] (pass-through + statistic path).
 */
size_t igan_mbstd_workspace_floats(int N, int H, int W, int C, int G);
int igan_mbstd_fwd(igan_stream_t stream, const float* x, float* y, float* workspace,
                   int N, int H, int W, int C, int G);
int igan_mbstd_bwd(igan_stream_t stream, const float* x, const float* dy, float* dx,
                   int N, int H, int W, int C, int G);

/* ------------------------------------------------------------------------
 * Exact streaming 1-nearest-neighbour (replaces dci_add + dci_query as used at
 * training/training_loop.py:367-368,398 with num_neighbours = 1).
 *   (best_d2[q], best_idx[q]) = lexicographic min over candidates c of (|query_q - cand_c|^2, idx_base + c)
 * with the squared distance of the winner -- and of every candidate that could be the winner -- computed
 * as a direct difference in fp64 (compute_dist, dci_code/src/util.c:62-69, before its sqrt), i.e. the
 * result equals an fp64 brute-force search (ties go to the lower index).  The fp32 MFMA product
 * |q|^2 + |c|^2 - 2 q.c only screens: candidates whose error interval (relative half-width
 * (dim + 2) * 2^-24, a rounding-error bound, of |q|^2 + |c|^2) cannot reach the best known upper bound are dropped, the rest are
 * measured exactly.  Initialise best_d2 to +infinity and best_idx to INT32_MAX; candidates can be streamed
 * batch after batch with increasing idx_base, the running minimum is order-independent, so the result is
 * deterministic.  A candidate with a non-finite product or distance never wins.
 * qnorm / cnorm are the squared row norms (igan_row_sqnorm, fp64 accumulate).  The caller takes sqrt
 * (Euclidean distance) of best_d2.
 */
int igan_row_sqnorm(igan_stream_t stream, const float* a, float* out, int rows, int dim);
int igan_nn1_update(igan_stream_t stream, const float* query, const float* qnorm,
                    const float* cand, const float* cnorm, double* best_d2, int* best_idx,
                    float* dots /* caller workspace, nq*nc floats */,
                    int nq, int nc, int dim, int idx_base);

/* ------------------------------------------------------------------------
 * Exact streaming k-nearest-neighbours with indices (replaces dci_query(num_neighbours = k) as the exclusive IMLE
 * assignment uses it, training/training_loop.py:382-396).  After any sequence of calls
 *   (best_d2[q][0..k), best_idx[q][0..k)) = the k lexicographically smallest pairs (|query_q - cand_c|^2, idx_base + c)
 * over all candidates fed so far, ascending, ties in distance to the lower index, with the squared distance of
 * igan_nn1_update (a direct difference in fp64); the fp32 MFMA product screens with the same error interval and every
 * pair it cannot rule out is measured exactly.  Initialise best_d2 to +infinity and best_idx to INT32_MAX.  The state is a
 * function of the set of (row, index) pairs fed -- not of the order or the boundaries of the batches, bits of the distances
 * included -- and with k = 1 it is igan_nn1_update's, bit for bit, as long as no screening value is NaN.  The two differ for
 * a candidate whose fp32 product or norms overflow (rows of magnitude ~1e19 and beyond), so that |q|^2 + |c|^2 - 2 q.c is
 * NaN, and whose exact distance is finite: igan_nn1_update never measures such a candidate and it never wins; igan_nnk_update
 * (like the manifold entries and igan_kmeans_step) measures it and it enters on its fp64 distance.  A candidate whose exact
 * distance is not finite never enters; with fewer than k finite candidates the trailing slots stay (+infinity, INT32_MAX).
 * 1 <= k <= 16 (IGAN_ERR_UNSUPPORTED beyond); non-null buffers, positive sizes, idx_base >= 0 and idx_base + nc <=
 * INT32_MAX, the operand limits of igan_conv2d (IGAN_ERR_INVALID_ARGUMENT).  Arguments are validated before anything
 * touches a device.
 */
int igan_nnk_update(igan_stream_t stream, const float* query, const float* qnorm,
                    const float* cand, const float* cnorm,
                    double* best_d2 /* [nq][k] */, int* best_idx /* [nq][k] */,
                    float* dots /* caller workspace, nq*nc floats */,
                    int nq, int nc, int dim, int k, int idx_base);

/* ------------------------------------------------------------------------
 * Exact k-NN manifold search for the precision / recall metric (reference: metrics/precision_recall.py).
 * Both entries take the products of one candidate batch from the exact-fp32 MFMA like igan_nn1_update
 * (dots: caller workspace, nq*nc floats), screen with |q|^2 + |c|^2 - 2 q.c and its error interval (relative
 * half-width (dim + 2) * 2^-24, a rounding-error bound, of |q|^2 + |c|^2) and measure every pair the interval cannot decide as a
 * direct difference in fp64 -- the squared distance of igan_nn1_update, symmetric, 0 for identical rows.
 * A non-finite exact distance counts as +infinity and is never within a radius.  Candidate batches may be
 * streamed in any order; the results do not depend on it.  1 <= kcap <= 16, 1 <= nk <= 8; the operand
 * limits are those of igan_conv2d.
 *
 * igan_knn_radius_update: folds the batch into each query's kcap smallest exact squared distances
 * (kth_d2 [nq][kcap], ascending, a multiset: duplicates count; initialise to +infinity).  Fed every point of
 * the query's own set, itself included, kth_d2[q][k] is what np.partition(distance_batch, seq)[:, k] leaves
 * at 0-based position k (precision_recall.py:76,90), without the [10 000 x n] fp16 host block (:75).
 *
 * igan_manifold_member_update: sets member[q][s] = 1 (member [nq][nk]; initialise to 0; never cleared) when a
 * candidate c of the batch has d2(q, c) <= cand_radius[c][s] (precision_recall.py:119-120, note the <=).
 * A query already marked in every column skips the batch.
 */
int igan_knn_radius_update(igan_stream_t stream, const float* query, const float* qnorm,
                           const float* cand, const float* cnorm,
                           double* kth_d2 /* [nq][kcap] ascending, caller-initialised to +inf */,
                           float* dots /* caller workspace, nq*nc floats */,
                           int nq, int nc, int dim, int kcap);
int igan_manifold_member_update(igan_stream_t stream, const float* query, const float* qnorm,
                                const float* cand, const float* cnorm,
                                const double* cand_radius /* [nc][nk] */,
                                int* member /* [nq][nk], caller-initialised to 0 */,
                                float* dots /* caller workspace, nq*nc floats */,
                                int nq, int nc, int dim, int nk);

/* igan_manifold_member_nn1_update: membership AND nearest neighbour of one candidate batch on ONE product block.  Its effect
 * on member, best_d2 and best_idx is, bit for bit, that of igan_manifold_member_update followed by igan_nn1_update on the
 * same arguments, with the product formed once (the precision pass of pr50k3 with realism / nearest index asks for both).
 * Each half keeps its own rules: a query marked in every column skips the membership walk but not the nearest-neighbour
 * one; the 1-NN drops a candidate its interval cannot decide, the membership test measures it.  The checks are those of the
 * two entries: non-null buffers, the operand limits of igan_conv2d, 1 <= nk <= 8, idx_base >= 0 and idx_base + nc <=
 * INT32_MAX (IGAN_ERR_INVALID_ARGUMENT), made before anything touches a device.
 */
int igan_manifold_member_nn1_update(igan_stream_t stream, const float* query, const float* qnorm,
                                    const float* cand, const float* cnorm,
                                    const double* cand_radius /* [nc][nk] */,
                                    int* member /* [nq][nk], caller-initialised to 0 */,
                                    double* best_d2 /* [nq], caller-initialised to +inf */,
                                    int* best_idx /* [nq], caller-initialised to INT32_MAX */,
                                    float* dots /* caller workspace, nq*nc floats */,
                                    int nq, int nc, int dim, int nk, int idx_base);

/* igan_ball_count_update: how many candidates lie inside each QUERY's own balls -- the count behind density and coverage
 * (Naeem et al., "Reliable Fidelity and Diversity Metrics for Generative Models", ICML 2020, the `prdc` definitions; the
 * reference has no such metric).  For every query q and column s it ADDS to count[q][s] the number of candidates c of the
 * batch with
 *   d2(q, c) <  query_radius[q][s]     (inclusive = 0: prdc's strict comparison)
 *   d2(q, c) <= query_radius[q][s]     (inclusive = 1: the comparison of igan_manifold_member_update)
 * on the exact squared distance of the entries above: the fp32 MFMA product screens with the same error interval, a pair whose
 * whole interval is on one side of the radius is decided by it, every other pair is measured as a direct difference in fp64.
 * The radii belong to the queries (squared, fp64, typically igan_knn_radius_update's), not to the candidates.  No early exit,
 * no atomic, no floating-point sum: count is a function of the multiset of (query, candidate) pairs fed, so candidate batches
 * may be streamed in any order and cut anywhere, and a batch fed twice counts twice.  Initialise count to 0.  A pair whose
 * exact distance is not finite is never counted and changes no other pair; a NaN or negative radius counts nothing; radius
 * +infinity counts every candidate at a finite distance; an interval that is NaN (overflowed fp32 products or norms) decides
 * nothing and the pair is measured.  Non-null buffers, the operand limits of igan_conv2d (an empty batch is refused),
 * 1 <= nk <= 8, inclusive 0 or 1 (IGAN_ERR_INVALID_ARGUMENT), checked before anything touches a device.
 */
int igan_ball_count_update(igan_stream_t stream, const float* query, const float* qnorm,
                           const double* query_radius /* [nq][nk] squared, fp64 */,
                           const float* cand, const float* cnorm,
                           long long* count /* [nq][nk], ADDED to */,
                           float* dots /* caller workspace, nq*nc floats */,
                           int nq, int nc, int dim, int nk, int inclusive /* 0: e < R, 1: e <= R */);

/* ------------------------------------------------------------------------
 * One exact k-means step for the PRD metric (reference: precision-recall-distributions/prd_score.py:125-127, the
 * MiniBatchKMeans behind _cluster_into_bins): the nearest centre of every row and the per-centre sums of the rows.
 *   (d2[i], label[i]) = lexicographic min over centres j of (|X_i - C_j|^2, j)
 * with the squared distance of igan_nn1_update: the exact-fp32 MFMA product |x|^2 + |c|^2 - 2 x.c only screens (relative
 * half-width (dim + 2) * 2^-24, a rounding-error bound, of |x|^2 + |c|^2), every centre the interval cannot rule out is measured as a direct
 * difference in fp64 -- labels and d2 equal an fp64 brute force on the same fp32 rows, ties go to the lower index.  A row
 * whose distances are all non-finite gets label -1 and d2 = +infinity and contributes to nothing below.
 *   sums[j] = sum of X_i over label[i] == j, count[j] = the number of such rows, inertia[0] = sum of d2[i] over labelled rows
 * all fp64, written (not accumulated); an empty cluster has count 0 and zero sums.  The order of every sum is a function of
 * (n, k, dim) alone and there is no floating-point atomic: two calls give the same bits.
 * xnorm / cnorm are the squared row norms (igan_row_sqnorm).  1 <= k <= 64 and 1 <= dim <= 4096 (IGAN_ERR_UNSUPPORTED
 * beyond either); non-null buffers, n >= 1, n * dim * 4 below 2 GiB and n * k within int32 (IGAN_ERR_INVALID_ARGUMENT:
 * longer row sets go in chunks, the caller adds the chunk results).  Arguments are validated before anything touches a
 * device.  workspace: igan_kmeans_workspace_bytes(n, k, dim) bytes (0 for sizes outside the limits), 16-byte aligned,
 * contents irrelevant.
 */
size_t igan_kmeans_workspace_bytes(int n, int k, int dim);
int igan_kmeans_step(igan_stream_t stream, const float* X /* [n][dim] */, const float* xnorm, const float* C /* [k][dim] */,
                     const float* cnorm, int* label /* [n] */, double* d2 /* [n] */, double* sums /* [k][dim] */,
                     long long* count /* [k] */, double* inertia /* [1] */, void* workspace, int n, int k, int dim);

/* ------------------------------------------------------------------------
 * Streaming mean / covariance of feature rows for the FID metric (reference: metrics/frechet_inception_distance.py:43-44,64-65,
 * np.mean and np.cov(rowvar=False) of the [num_images, 2048] activation block).  Added without a version bump: three more
 * exports, no struct or signature changes.  Arguments are validated before anything touches a device.
 *
 * igan_moments_update ACCUMULATES one batch into caller-zeroed running statistics.  With d_ij = (double)X[i][j] - shift[j]
 * (shift == NULL: 0):   sum[j] += sum_i d_ij,   gram[j][k] += sum_i d_ij * d_ik for j <= k; the lower triangle of gram is
 * unspecified until finalize.  The conversion is exact, the subtraction rounds once, products and accumulation are fp64 on
 * v_mfma_f64_16x16x4_f64 and sum is fp64 too.  Every 64 x 64 tile on or above the diagonal is owned by one workgroup, which
 * walks the n rows in order and does the read-modify-write of its tile itself -- no split over n, no floating-point atomic:
 * the bits are a function of (n, F) and the sequence of calls, and a repeated sequence gives identical bits.  Rows past n
 * and columns past F contribute an exact 0 (the SHIFTED value is padded).  A NaN or infinity in X[i][j] reaches sum[j] and
 * row / column j of gram as IEEE gives it and nothing else.  1 <= F <= 4096 (IGAN_ERR_UNSUPPORTED beyond); n >= 1, non-null
 * X / sum / gram and n * F * 4 below 2 GiB (IGAN_ERR_INVALID_ARGUMENT; longer row sets go in several calls).  X needs 4-byte
 * alignment only, shift / sum / gram 8-byte.  workspace: igan_moments_workspace_bytes(n, F) bytes -- 0 in this design, the
 * pointer may be NULL.
 *
 * igan_moments_finalize WRITES, in fp64,   mean[j] = shift[j] + sum[j] / n_total   and, for j <= k,
 *     cov[j][k] = cov[k][j] = (gram[j][k] - sum[j] * sum[k] / n_total) / (n_total - 1)             n_total >= 2
 * With the shift near the mean the correction term is tiny and nothing cancels: on features 100 + 0.01 N(0, 1) a zero shift
 * is wrong by 3.6e-7 of sqrt(cov_jj cov_kk), the mean of the first 8 rows as the shift by 1.4e-16.  cov must not alias gram.
 *
 * igan_moments_merge (one more export under version 10) FOLDS state B -- n_b rows about shift_b -- into state A, re-expressed
 * about A's shift, without reading a feature row again: with dl_j = shift_b[j] - shift_a[j] (a NULL shift is 0)
 *     sum_a[j]     += sum_b[j] + n_b dl_j
 *     gram_a[j][k] += gram_b[j][k] + dl_j sum_b[k] + sum_b[j] dl_k + n_b dl_j dl_k                  for j <= k only
 * This is how the statistics of several ranks become one (FeatureMoments.all_merge: every rank folds the ranks' states in
 * rank order and ends with the same bits).  All fp64; one thread owns each output element of the 64 x 64 tiles on or above
 * the diagonal (the diagonal tile's workgroup owns sum), no atomic and no reduction: the bits are a function of the inputs
 * alone.  The lower triangle of gram_a stays unspecified until finalize; the strict lower triangle of gram_b is never read;
 * B is not written, shift_a is not changed and the caller adds the counts.  A non-finite sum_b[j], gram_b[j][.] or
 * shift_*[j] reaches sum_a[j] and row / column j of gram_a and nothing else: every operand of element (j, k) carries index
 * j or k.  F > 4096: IGAN_ERR_UNSUPPORTED; F < 1, n_b < 1, a null sum / gram, sum_a == sum_b, gram_a == gram_b or a pointer
 * that is not 8-byte aligned: IGAN_ERR_INVALID_ARGUMENT. */
size_t igan_moments_workspace_bytes(int n, int F);
int igan_moments_update(igan_stream_t stream, const float* X /* [n][F] row-major */, const double* shift /* [F] or NULL */,
                        double* sum /* [F] */, double* gram /* [F][F] */, void* workspace, size_t workspace_bytes, int n, int F);
int igan_moments_finalize(igan_stream_t stream, const double* sum, const double* gram, const double* shift /* or NULL */,
                          double* mean /* [F] */, double* cov /* [F][F] */, long long n_total, int F);
int igan_moments_merge(igan_stream_t stream, double* sum_a, double* gram_a, const double* shift_a /* [F] or NULL = 0 */,
                       const double* sum_b, const double* gram_b, const double* shift_b /* [F] or NULL = 0 */, long long n_b, int F);

/* ------------------------------------------------------------------------
 * Pair sums of the cubic polynomial kernel for the Kernel Inception Distance (kid50k; Binkowski et al., "Demystifying MMD
 * GANs", ICLR 2018; the reference has no such metric).  Two more exports under version 10.  With
 *   k(a, b) = (gamma * a.b + coef0)^3,   x_i = X[idx_x[s][i]],   y_j = Y[idx_y[s][j]]   (i, j positions in [0, m))
 * igan_poly3_kernel_sums OVERWRITES, for every subset s of the S subsets,
 *   out[s][0] = sum over i != j of k(x_i, x_j)     out[s][1] = sum over i != j of k(y_i, y_j)     out[s][2] = sum over all i, j of k(x_i, y_j)
 * The diagonal that the two symmetric sums skip (it is skipped, not subtracted) is the diagonal of POSITIONS: a subset that
 * lists one row twice at two positions counts that pair.  X and Y may be the same matrix.
 * Arithmetic: every fp32 feature is widened to fp64 before any product, the dot products accumulate in fp64 on
 * v_mfma_f64_16x16x4_f64 four features per instruction, the instructions in ascending feature order, v = fma(gamma, dot, coef0) and (v * v) * v are fp64; no fp32 value is
 * formed after the load.  Rows are gathered by index while they are staged; no copy of a subset exists.  One workgroup owns a
 * 64 x 64 tile of one pair matrix of one subset (tiles on or above the diagonal for the symmetric sums, a tile strictly above
 * it counted twice), adds its cells in a fixed order -- lane-local, the xor tree of a wavefront, the four wavefronts in order
 * -- into ONE fp64 of `partials`, and a second kernel adds the partials of a (subset, sum) serially in tile order: no atomic,
 * no split over F.  out[s] is a function of subset s's indices and features only: the same bits launched alone or among
 * others, on every run, whatever `partials` held.  A NaN or infinity in a row reaches only the sums of the subsets that list
 * that row (sums 0 and 2 for a row of X, 1 and 2 for a row of Y); a subset that does not list it is bit-identical.
 * INDICES ARE NOT RANGE-CHECKED on the device: the caller owns 0 <= idx_x < nx and 0 <= idx_y < ny (the Python binding checks
 * on the host before it uploads); nx and ny are validated as sizes only.
 * Limits: 1 <= F <= 4096 and S * m and S * (2 T^2 + T) tiles, T = ceil(m / 64), below 2^31 (IGAN_ERR_UNSUPPORTED beyond);
 * S >= 1, m >= 2, nx >= 1, ny >= 1, non-null buffers, X / Y / idx_* 4-byte and partials / out 8-byte aligned
 * (IGAN_ERR_INVALID_ARGUMENT), all checked before a launch.  partials: igan_poly3_kernel_sums_workspace_bytes(S, m) bytes
 * (0 for sizes outside the limits), contents irrelevant before and after. */
size_t igan_poly3_kernel_sums_workspace_bytes(int S, int m);
int igan_poly3_kernel_sums(igan_stream_t stream, const float* X /* [nx][F] row-major */, int nx, const float* Y /* [ny][F] */, int ny,
                           const int* idx_x /* [S][m] rows of X */, const int* idx_y /* [S][m] rows of Y */, int S, int m, int F,
                           double gamma, double coef0, double* partials /* workspace */, double* out /* [S][3] */);

/* ------------------------------------------------------------------------
 * Per-class statistics of classifier outputs, folded batch by batch on the device.  Added without a version bump: two more
 * exports, no struct or signature changes.  Arguments are validated before anything touches a device: a null logits / counts
 * / probs / psum / plogp, n < 1, K < 1, n * K * 4 at or above 2 GiB (longer row sets go in several calls), counts / psum /
 * plogp not 8-byte aligned or an input not 4-byte aligned return IGAN_ERR_INVALID_ARGUMENT.  Inputs are dense row-major fp32
 * and need 4-byte alignment ONLY: a row of an odd K starts anywhere, the kernels' 16-byte loads are declared 4-byte aligned.
 *
 * igan_class_hist_update replaces np.argmax(logits, axis=1) and the label array np.unique / np.histogram read on the host
 * (reference: metrics/mode_counts.py:41-46, metrics/KL.py:41-49).  label[i] is np.argmax(logits[i]) exactly: the lowest index
 * among equal maxima with -0.0 == +0.0, the index of the first NaN of a row that holds one, 0 for a row of -infinity; then
 * counts[label[i]] += 1 into caller-zeroed running counts.  labels may be NULL.  One wavefront per row; a workgroup adds the
 * multiplicity of each distinct label of its 16 rows with one 64-bit INTEGER atomic, so the counts do not depend on order.
 *
 * igan_prob_stats_update replaces the host activation block of the Inception Score (reference: metrics/inception_score.py:
 * 43-54): it ACCUMULATES, in fp64 and as IEEE gives it,
 *     psum[k] += sum_i (double)probs[i][k]          plogp[0] += sum_i sum_k (double)probs[i][k] * log((double)probs[i][k])
 * from which a split's score is exp(plogp / n - sum_k m_k log m_k), m = psum / n.  A zero contributes 0 * -inf = NaN to
 * plogp, a negative or NaN probability NaN (the reference's statement gives NaN for such a split too); psum of the other
 * columns is untouched by it.  One thread owns a psum column and walks the rows in order; a row's plogp terms are summed per
 * lane in ascending column order, over the lanes in a fixed tree, and one thread adds the row sums in row order -- no
 * floating-point atomic: the bits are a function of (n, K) and the sequence of calls, and a repeated sequence gives
 * identical bits.  The kernel knows nothing about splits: the caller cuts a batch at split boundaries. */
int igan_class_hist_update(igan_stream_t stream, const float* logits /* [n][K] */, long long* counts /* [K], accumulated */,
                           int* labels /* [n] or NULL */, int n, int K);
int igan_prob_stats_update(igan_stream_t stream, const float* probs /* [n][K] */, double* psum /* [K], accumulated */,
                           double* plogp /* [1], accumulated */, int n, int K);

/* ------------------------------------------------------------------------
 * Softmax cross-entropy against integer labels: the loss of the Stacked-MNIST mode classifier this project trains for itself
 * (the reference ships no trainer for metrics/stacked_mnist_classifier.pkl, metrics/mode_counts.py:29).  Added without a
 * version bump: three more exports, no struct or signature changes.  Arguments are validated before anything touches a
 * device: a null pointer (pred of the forward alone may be NULL), n < 1, K < 1, n * K * 4 at or above 2 GiB, lse / loss_sum /
 * counts not 8-byte aligned or another buffer not 4-byte aligned return IGAN_ERR_INVALID_ARGUMENT.  Inputs are dense
 * row-major and need 4-byte alignment ONLY: a row of an odd K starts anywhere.  No workspace, no floating-point atomic: the
 * bits are a function of (n, K), the data and the sequence of calls.
 *
 * igan_softmax_xent_fwd / _bwd replace torch.nn.functional.cross_entropy(logits, labels, reduction='none') and its
 * gradient, as fp64 states them:
 *     lse[i]  = m + log sum_k exp((double)x[i][k] - m),  m = max_k x[i][k]        evaluated and STORED in fp64
 *     loss[i] = (float)(lse[i] - x[i][label[i]])
 *     dlogits[i][k] = (float)(dloss[i] * (exp((double)x[i][k] - lse[i]) - (k == label[i])))     one rounding, from the stored lse
 * (lse is evaluated as m + log1p(sum over k != argmax of exp(x[i][k] - m)) -- the arg-max column's term is exactly 1, and the
 * logarithm of a sum rounded next to 1 would lose the digits of a confident row's lse -- and exp(a) - 1 at the label's column
 * as expm1(a): a confident row has p within a few ulp of 1 there.)
 * A row whose label lies outside [0, K) is ignored (the trainer pads with -1): loss 0, gradient row 0, nothing is read at the
 * label's column; its lse and pred are still written.  pred[i] is np.argmax(x[i]) under exactly the rules of
 * igan_class_hist_update (lowest index among equal maxima, the first NaN, 0 for a row of -infinity).  Non-finite values stay
 * in their own row: a NaN or +infinity logit, or a row of -infinity, makes that row's lse, loss and gradient row NaN and
 * changes no other row; a -infinity among finite logits contributes exactly 0.  Forward: one wavefront per row, lane sums in
 * ascending column order, then a fixed tree over the lanes.  Backward: one thread per element.
 *
 * igan_xent_stats_update ACCUMULATES the numbers a trainer tick reports, over the rows whose label lies in [0, K):
 *     loss_sum[0] += sum_i (double)loss[i]  in row order, by one owner        counts[0] += rows counted        counts[1] += rows with pred[i] == label[i]
 * so the mean loss and accuracy of a tick are one device -> host copy.  A NaN loss makes loss_sum NaN, as the sum does. */
int igan_softmax_xent_fwd(igan_stream_t stream, const float* logits /* [n][K] */, const int* labels /* [n] */, float* loss /* [n] */,
                          double* lse /* [n] */, int* pred /* [n] or NULL */, int n, int K);
int igan_softmax_xent_bwd(igan_stream_t stream, const float* logits /* [n][K] */, const int* labels /* [n] */, const double* lse /* [n] */,
                          const float* dloss /* [n] */, float* dlogits /* [n][K] */, int n, int K);
int igan_xent_stats_update(igan_stream_t stream, const float* loss /* [n] */, const int* labels /* [n] */, const int* pred /* [n] */,
                           double* loss_sum /* [1], accumulated */, long long* counts /* [2]: rows counted, rows correct; accumulated */,
                           int n, int K);

/* ------------------------------------------------------------------------
 * Sigmoid (binary) cross-entropy against {0, 1} targets, A independent attributes per row: the loss of the CelebA attribute
 * classifier this project trains for itself (the reference downloads 40 classifiers, metrics/linear_separability.py:20-61,
 * from URLs this tree never opens), and the probability pairs linear separability takes from it.  Added without a version
 * bump: four more exports, no struct or signature changes.  Arguments are validated before anything touches a device: a null
 * pointer (pos_weight, and pred of the forward, may be NULL), n < 1, A < 1, n * A * 4 at or above 2 GiB, loss_sum / counts /
 * probs not 8-byte aligned or another float buffer not 4-byte aligned return IGAN_ERR_INVALID_ARGUMENT.  Inputs are dense
 * row-major and need 4-byte alignment ONLY: a row of an odd A starts anywhere.  No workspace, no floating-point atomic: the
 * bits are a function of (n, A), the data and the sequence of calls.
 *
 * igan_sigmoid_xent_fwd / _bwd replace torch.nn.functional.binary_cross_entropy_with_logits(logits, targets,
 * pos_weight=pos_weight, reduction='none') and its gradient, as fp64 states them.  With x = (double)logits[i][a],
 * w = pos_weight[a] (1 when the pointer is NULL) and softplus(z) = max(z, 0) + log1p(exp(-|z|)) in fp64, by the element's target t:
 *     t == 1.0f  positive    loss = (float)(w * softplus(-x))      dlogits = (float)(dloss * (-w / (1 + exp(x))))
 *     t == 0.0f  negative    loss = (float)(softplus(x))           dlogits = (float)(dloss * (1 / (1 + exp(-x))))
 *     otherwise  ignored     loss = 0                              dlogits = 0        (NaN and the trainer's padding -1 included)
 *     pred[i][a] = x > 0                                                              (a NaN predicts 0)
 * each result rounded to fp32 once.  The gradient is NOT sigmoid(x) - t: a confident correct element keeps every digit of its
 * small gradient.  A NaN logit gives a NaN loss and gradient (the max is a comparison and does not swallow it); +infinity
 * with a positive target gives loss 0 (softplus(-inf) = 0, never inf - inf) and gradient -0 * dloss, with a negative target
 * loss +infinity.  A non-finite logit changes its own element only.  One thread per element.
 *
 * igan_sigmoid_xent_stats_update ACCUMULATES the numbers a trainer tick reports per attribute a, over the elements that are not ignored:
 *     loss_sum[a] += sum_i (double)loss[i][a]   one owner per column, rows in ascending order, ONE fp64 accumulator
 *     counts[a][0..3] += (tp, fp, tn, fn)        positive & pred, negative & pred, negative & !pred, positive & !pred, pred = logits > 0
 * so the mean loss, accuracy and balanced accuracy of every attribute are one device -> host copy.  A NaN loss makes that
 * column's loss_sum NaN, as the sum does.
 *
 * igan_binary_probs replaces softmax(concat([logits, -logits], axis=1)) of linear_separability.py:138 for ALL attributes of a
 * [n][A] logit matrix in one pass:
 *     probs[a][i][0] = (float)(1 / (1 + exp(-2 x)))      probs[a][i][1] = (float)(1 / (1 + exp(2 x)))      (x - (-x) = 2 x)
 * attribute-major, so that attribute a's [n][2] block is contiguous.  fp64 from the fp32 logit, one rounding each; NaN gives
 * (NaN, NaN), +infinity (1, 0). */
int igan_sigmoid_xent_fwd(igan_stream_t stream, const float* logits /* [n][A] */, const float* targets /* [n][A] */,
                          const float* pos_weight /* [A] or NULL */, float* loss /* [n][A] */, int8_t* pred /* [n][A] or NULL */, int n, int A);
int igan_sigmoid_xent_bwd(igan_stream_t stream, const float* logits /* [n][A] */, const float* targets /* [n][A] */,
                          const float* pos_weight /* [A] or NULL */, const float* dloss /* [n][A] */, float* dlogits /* [n][A] */, int n, int A);
int igan_sigmoid_xent_stats_update(igan_stream_t stream, const float* loss /* [n][A] */, const float* logits /* [n][A] */,
                                   const float* targets /* [n][A] */, double* loss_sum /* [A], accumulated */,
                                   long long* counts /* [A][4]: tp, fp, tn, fn; accumulated */, int n, int A);
int igan_binary_probs(igan_stream_t stream, const float* logits /* [n][A] */, float* probs /* [A][n][2] */, int n, int A);

/* ------------------------------------------------------------------------
 * Perceptual path length (reference: metrics/perceptual_path_length.py; ppl_zfull .. ppl2_wend).  Added without a
 * version bump: two more exports, no struct or signature changes.
 *
 * igan_ppl_endpoints replaces normalize / slerp (:19-30) and the endpoint expressions (:59-77): for pair i with ends
 * lat[2i], lat[2i+1] ([2n][dim] fp32) and position t[i] it writes the point at t[i] to out[2i] and the point at
 * t[i] + epsilon to out[2i+1] -- the interleaving of :71,76.  mode 0: lerp a + (b - a) * t (dim = num_layers *
 * dlatent_size); mode 1: the reference's slerp (three normalisations, acos, cos, sin).  The arithmetic is fp64 from the
 * fp32 inputs, t + epsilon included, and each output is rounded to fp32 once: the two rows of a pair differ by about
 * epsilon of their size and the metric divides by epsilon^2, so an fp32 evaluation would put ~1e-3 relative error into
 * the difference before G runs.  lerp is three uncontracted fp64 operations (numpy's result bit for bit).  Degenerate
 * pairs (a parallel to b, a zero row) give what the formula gives, NaN included, as in the reference.  Any dim >= 1;
 * 16-byte accesses when dim % 4 == 0 and both buffers are 16-byte aligned.  out must not overlap lat.
 *
 * igan_ppl_crop_prep replaces :84-96 (crop, box-mean downsample, range change) in one pass.  x is G's fp32 image batch
 * addressed through ELEMENT STRIDES, x[n][c][h][w] at n*stride_n + c*stride_c + h*stride_h + w*stride_w, so whatever
 * layout G_synthesis hands back is read in place.  The window is rows y0:y1, columns x0:x1; factor >= 1 divides both
 * sides.  y is [N][(y1-y0)/factor][(x1-x0)/factor][C] channel-minor, 16-byte aligned:
 *     y = (m + 1) * (255 / 2),   m = (sum of the factor x factor box in fp32, rows then columns) * (1 / factor^2)
 * uncontracted and without a clamp (the reference has none); factor == 1 gives fp32 (x + 1) * 127.5 bit for bit. */
int igan_ppl_endpoints(igan_stream_t stream, const float* lat, const float* t, float* out, int n, int dim,
                       double epsilon, int mode);
int igan_ppl_crop_prep(igan_stream_t stream, const float* x, float* y, int N, int C, int H, int W,
                       int y0, int y1, int x0, int x1, int factor,
                       long long stride_n, long long stride_c, long long stride_h, long long stride_w);

/* ------------------------------------------------------------------------
 * Batched primal linear SVM for the linear separability metric (reference: metrics/linear_separability.py:162-165,
 * sklearn.svm.LinearSVC() at its defaults: squared hinge, L2, C = 1, the bias a regularised extra feature of value 1).
 * Added without a version bump: more exports, no struct or signature changes.
 *
 *     f_a(w) = 1/2 |w|^2 + C * sum_{i : Y[i][a] != 0} max(0, 1 - Y[i][a] * w.(x_i, 1))^2        w in R^(F+1), bias last
 *
 * X [n][F] fp32 row-major is shared by all A attributes; Y [n][A] int8 holds -1 / +1, 0 = the attribute has pruned the
 * sample.  1 <= A <= 64 per launch (larger sets go in groups), 1 <= F <= 1024 (IGAN_ERR_UNSUPPORTED beyond either),
 * n * F * 4 below 2 GiB and n * A within int32 (IGAN_ERR_INVALID_ARGUMENT).  Arguments are validated before anything
 * touches a device.  One pass reads X from HBM once and uses each 32-row slab for both products on the exact-fp32 MFMA;
 * sums over n are per-workgroup partials added in a fixed order in fp64 -- no atomics, the same inputs give the same bits.
 * workspace: igan_linear_svc_workspace_bytes(n, F, A) bytes (0 for sizes outside the limits), contents irrelevant.
 *
 * igan_linear_svc_grad (:162-163, the fit): dec[i][a] = W[a].(x_i, 1); m = 1 - y dec; active[i][a] = (y != 0 && m > 0);
 *     loss[a] = sum of m^2 over active samples; grad[a] = -2C * sum_i active y m (x_i, 1)   (the caller adds W[a]).
 * igan_linear_svc_hv (:162-163): z[i][a] = S[a].(x_i, 1); hv[a] = 2C * sum_i active z (x_i, 1)   (the caller adds S[a]);
 *     active is the mask the last igan_linear_svc_grad stored.
 * igan_linear_svc_linesearch (:162-163): out[k][a] = sum_{y != 0} max(0, 1 - y (dec + t[k][a] z))^2 for 1 <= T <= 8 step
 *     sizes per attribute, from dec and z alone (dec(w + t s) = dec(w) + t z), evaluated in fp64; X is not read.
 * igan_linear_svc_predict (:164-165, score / predict): pred[i][a] = (dec[i][a] > 0). */
size_t igan_linear_svc_workspace_bytes(int n, int F, int A);
int igan_linear_svc_grad(igan_stream_t stream, const float* X, const signed char* Y, const float* W /* [A][F+1] */,
                         float* dec /* [n][A] */, unsigned char* active /* [n][A] */, double* loss /* [A] */,
                         double* grad /* [A][F+1] */, void* workspace, size_t workspace_bytes, int n, int F, int A, double C);
int igan_linear_svc_hv(igan_stream_t stream, const float* X, const unsigned char* active, const float* S /* [A][F+1] */,
                       float* z /* [n][A] */, double* hv /* [A][F+1] */, void* workspace, size_t workspace_bytes,
                       int n, int F, int A, double C);
int igan_linear_svc_linesearch(igan_stream_t stream, const float* dec, const float* z, const signed char* Y,
                               const double* t /* [T][A] */, double* out /* [T][A] */, void* workspace, size_t workspace_bytes,
                               int n, int A, int T);
int igan_linear_svc_predict(igan_stream_t stream, const float* dec, int* pred /* [n][A] */, int n, int A);

/* ------------------------------------------------------------------------
 * fp32 image batch <-> uint8 (reference: dnnlib/tflib/tfutil.py:245-267, convert_images_from_uint8 / convert_images_to_uint8:
 * the output transform of every generator script and the conversion in front of every metric's feature network).  Added without a
 * version bump: two more exports, no struct or signature changes.  Arguments are validated before anything touches a device.
 *
 * igan_images_to_uint8 replaces :255-267 (cast, avg_pool, transpose, scale + bias, saturate_cast) in one pass.  x is addressed
 * through ELEMENT STRIDES, x[n][c][h][w] at n*stride_n + c*stride_c + h*stride_h + w*stride_w, so whatever layout G_synthesis hands
 * back (a view with an offset included) is read in place.  y is contiguous bytes, [N][H/shrink][W/shrink][C] when nhwc, else
 * [N][C][H/shrink][W/shrink]; the divisions floor, as VALID pooling does (a remainder of rows / columns is dropped).
 *     m = (sum of the shrink x shrink box in fp32, rows then columns) * fp32(1 / shrink^2);   shrink == 1: m = x itself
 *     v = m * scale + bias      the multiply and the add are two fp32 roundings, NEVER contracted into a fused multiply-add:
 *                               values one ulp from (k - 128) / 127.5 -- where images that were uint8 once live -- give
 *                               another byte under one rounding than under the reference's two
 *     y = 0 for v < 0 or v == -inf;  255 for v >= 255 or v == +inf;  0 for NaN;  otherwise v truncated towards zero.
 * The reference leaves NaN to an undefined cast (saturate_cast clamps, and a clamped NaN stays NaN); this kernel DEFINES it as 0.
 * scale = 255 / (drange[1] - drange[0]) and bias = 0.5 - drange[0] * scale, computed by the caller in double and rounded once.
 * Limits (IGAN_ERR_INVALID_ARGUMENT otherwise): non-null buffers, shrink >= 1, C >= 1, N, H, W >= 1, H / shrink and W / shrink >= 1,
 * non-negative strides, N*C*H*W and the largest strided offset within int32.  C <= 4 are specialised; loads are 16-byte where
 * stride_w == 1 (or the pixels are dense and channel-minor) and the addresses are 16-byte aligned, scalar otherwise.
 *
 * igan_images_from_uint8 replaces :245-252: x is [N][C][H][W] bytes, or [N][H][W][C] when nhwc_in; y is contiguous NCHW fp32,
 *     y = float(x) * scale + bias       uncontracted; scale = (drange[1] - drange[0]) / 255, bias = drange[0]. */
int igan_images_to_uint8(igan_stream_t stream, const float* x, unsigned char* y, int N, int C, int H, int W, int shrink,
                         float scale, float bias, int nhwc,
                         long long stride_n, long long stride_c, long long stride_h, long long stride_w);
int igan_images_from_uint8(igan_stream_t stream, const unsigned char* x, float* y, int N, int C, int H, int W,
                           float scale, float bias, int nhwc_in);

/* ------------------------------------------------------------------------
 * Differentiable augmentation of the images D sees, reals and fakes (Zhao et al., "Differentiable Augmentation for Data-Efficient
 * GAN Training", NeurIPS 2020; the reference has no such step: training/augment.py, training/loss.py `augment=`).  Three more exports
 * under version 10, no struct.  Arguments are validated before anything touches a device.
 *
 * x, y: [n][h][w][c] fp32, 1 <= c <= 4.  u: [n][8] fp32 uniforms in [0, 1), one row per sample (column 7 is padding).  policy is a bit
 * set, 1 = color, 2 = translation, 4 = cutout, always applied in that order.  Integer parameters are derived on the device as
 *     draw(u, k) = min(floor(fl32(u * k)), k - 1)          the product rounded to fp32 (the clamp holds it below k whatever that rounding does)
 *   color        b = u0 - 1/2, s = 2 u1, c = u2 + 1/2;  m = mean of the sample's c h w inputs, summed in fp64 in a fixed order
 *                (csrc/diffaugment.hip states it) and rounded to fp32 once;  M = m + b;  per pixel xb_k = x_k + b, p = mean_k xb_k,
 *                    v_k = ((xb_k - p) s + p - M) c + M        (brightness, saturation, contrast; fp32, one rounding per operation)
 *   translation  S_y = floor(h / 8 + 1/2), t_y = draw(u4, 2 S_y + 1) - S_y; t_x likewise from u3 and w;
 *                    w(i, j) = v(i + t_y, j + t_x) where that lies inside the image, else exactly 0  (m is that of the untranslated image)
 *   cutout       K_y = floor(h / 2 + 1/2), r_y = 1 - K_y mod 2, o_y = draw(u6, h + r_y): rows o_y - K_y / 2 <= i < o_y - K_y / 2 + K_y
 *                are cut; columns likewise from u5 and w; a pixel whose row and column are both cut is exactly 0.
 * igan_diffaugment_bwd is the transpose: g(i, j) = dy(i - t_y, j - t_x) where that position is inside the image and not cut, else 0;
 * without color dx = g; with color Gm = mean of g over the sample (fp64 sum, rounded once), q = mean_k g_k,
 *     dx_k = (c s) g_k + (c (1 - s)) q + (1 - c) Gm.
 * A cut or shifted-out value is 0 whatever its source holds; without color kept values are bit copies (policy 0: a plain copy).  With
 * color a non-finite input makes every kept value of its own sample non-finite and touches no other sample.
 * Launches: one, or with color two (one reduction, one pass).  No allocation, no host read, no atomic: capturable, and the same inputs
 * give the same bits whatever n and the sample's place in the batch.
 * workspace: igan_diffaugment_workspace_bytes(n, c, h, w) bytes, 8-byte aligned, contents irrelevant; needed with color only (may be
 * NULL otherwise).  The size is 0 exactly for the shapes the entry points refuse with IGAN_ERR_UNSUPPORTED: c > 4, or n * c * h * w
 * at or beyond 2^31.  IGAN_ERR_INVALID_ARGUMENT: a null buffer, n, c, h or w < 1, unknown policy bits, y == x, x / y not aligned to
 * the pixel access (16 bytes for c = 4, 8 for c = 2, else 4). */
size_t igan_diffaugment_workspace_bytes(int n, int c, int h, int w);
int igan_diffaugment_fwd(igan_stream_t stream, const float* x, float* y, const float* u /* [n][8] */, int n, int c, int h, int w,
                         int policy, void* workspace);
int igan_diffaugment_bwd(igan_stream_t stream, const float* dy, float* dx, const float* u /* [n][8] */, int n, int c, int h, int w,
                         int policy, void* workspace);

/* ------------------------------------------------------------------------
 * Device-side time stamps (measurement support, not part of the reference's surface): igan_stamp writes the constant
 * 100 MHz counter (10 ns ticks) into *slot in stream order, so two stamps bracket whatever was launched between them --
 * also inside a captured hipGraph, where host events cannot be placed.  igan_stamp_accumulate adds, for pairs
 * first .. first+count-1, stamps[2i+1] - stamps[2i] into acc[i]; captured at the end of a graph it turns every replay
 * into one more sample per launch without host involvement. */
int igan_stamp(igan_stream_t stream, unsigned long long* slot);
/* Diagnostic: while p != NULL every igan_conv2d launch of the MFMA forward kernel writes, per workgroup, 4 ticks of the same
 * counter (kernel entry, main-loop start, main-loop end, exit) to p[4 * workgroup + k]; the buffer must hold 4 * grid words. */
void igan_debug_set_conv_diag(unsigned long long* p);
int igan_stamp_accumulate(igan_stream_t stream, const unsigned long long* stamps, unsigned long long* acc, int first, int count);

/* ------------------------------------------------------------------------
 * Flat-bucket optimizer step (dnnlib/tflib/optimizer.py:237-239,318-332):
 *   flag[0] = all(isfinite(grad));  if flag: Adam update; else: skip.
 *   m = b1*m + (1-b1)*g; v = b2*v + (1-b2)*g*g; w -= lr_t * m / (sqrt(v) + eps)
 * lr_t = lr * sqrt(1 - b2pow') / (1 - b1pow') with b?pow' = b?pow * beta? read from
 * the device-resident pow_state[2] = {b1pow, b2pow} (initialise to {1, 1}); the
 * powers advance only when the step is applied, like TF's beta-power slots, and
 * no host synchronisation is needed to learn whether it was.
 * igan_finite_check ORs a non-zero into flag[0] when any element is non-finite
 * (flag must be zeroed by the caller before the first check of a step).
 * igan_ema: dst = src + (dst - src) * beta  (Network.setup_as_moving_average_of,
 * dnnlib/tflib/network.py:341-351).
 */
int igan_finite_check(igan_stream_t stream, const float* g, int n, int* flag);
int igan_adam_step(igan_stream_t stream, float* w, const float* g, float* m, float* v,
                   int n, float lr, float beta1, float beta2, float eps,
                   float* pow_state, const int* skip_flag);
int igan_ema(igan_stream_t stream, float* dst, const float* src, int n, float beta);

/* Running mean of a training scalar (role of dnnlib/tflib/autosummary.py:45-74): acc[0] += number of finite values among
 * x[0..n), acc[1] += their sum (double accumulators that live across hipGraph replays; non-finite values are ignored, :64).
 * One launch, fixed-order reduction. */
int igan_summary_accumulate(igan_stream_t stream, const float* x, int n, double* acc);

#ifdef __cplusplus
}
#endif
#endif /* IGAN_HIP_H */
