/*
 * hp3d.h -- C-ABI of libhp3d.so: the MI355X (gfx950) engine behind the Python call
 * surface of lmb-freiburg/hand3d's ColorHandPose3DNetwork / PosePriorNetwork.
 *
 * The reference has no FFI of its own: its "operator API" is the method surface of two
 * Python classes whose arithmetic runs inside TensorFlow 1.3.  Each entry
 * point below names the reference interface it replaces (file:line relative to the
 * reference tree).  The reference-side binding (ctypes) is hand3d_amd/_lib.py and is
 * reproduced in INTEGRATION.md.
 *
 * Conventions
 *   - return 0 on success, a negative hp3d_status otherwise; hp3d_last_error() gives text;
 *   - no C++ exception crosses this boundary, no torch/TF types appear in it;
 *   - all tensors are float32, NHWC, contiguous (the reference's layout: utils/general.py:40-46);
 *   - "host" entry points take caller-owned host buffers, are synchronous and never retain
 *     a pointer; "_dev" entry points take device pointers (hipMalloc'd by anyone in this
 *     process, e.g. a torch tensor's data_ptr) and are stream-ordered on hp3d_stream(ctx):
 *     call hp3d_sync() before reading results;
 *   - any output pointer may be NULL (that output is then not copied out);
 *   - a context is thread-compatible: no concurrent calls on one context.
 */
#ifndef HP3D_H
#define HP3D_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hp3d_ctx hp3d_ctx;

typedef enum {
    HP3D_OK = 0,
    HP3D_ERR_ARG = -1,        /* bad argument / shape (the reference's bare asserts)            */
    HP3D_ERR_HIP = -2,        /* a HIP runtime call failed                                      */
    HP3D_ERR_WEIGHTS = -3,    /* missing / mis-shaped variable at finalize, or not finalized    */
    HP3D_ERR_UNSUPPORTED = -4,/* e.g. evaluation=False / train=True, unsupported geometry          */
    HP3D_ERR_NOMEM = -5
} hp3d_status;

/* PosePriorNetwork variants -- nets/PosePriorNetwork.py:59-95 */
enum { HP3D_VARIANT_DIRECT = 0, HP3D_VARIANT_BOTTLENECK = 1, HP3D_VARIANT_PROPOSED = 2,
       HP3D_VARIANT_LOCAL = 3 /* 'local' and 'local_w_xyz_loss': + bone_rel_trafo_inv, utils/relative_trafo.py:243-295 */ };
/* activation fused behind a conv / fc -- utils/general.py:55-59,132-136 */
enum { HP3D_ACT_NONE = 0, HP3D_ACT_LEAKY = 1 };

int hp3d_abi_version(void);
/* HIP devices visible to this process (hipGetDeviceCount); needs no context.  No reference counterpart (one tf.Session on whatever
 * device TensorFlow picks, run.py:44-50): a launcher uses it to refuse `--gpus N` on a box with fewer devices BEFORE any rank
 * starts, instead of leaving N - n ranks to fail one by one inside a rendezvous.  Returns 0 or HP3D_ERR_HIP (then *count = 0). */
int hp3d_device_count(int* count);
/* PCI address "dddd:bb:dd.f" of HIP device `device` (hipDeviceGetPCIBusId) into buf (cap >= 13); needs no context.  No reference
 * counterpart (same single-session script): a multi-rank launcher reads the device's NUMA node from
 * /sys/bus/pci/devices/<address>/numa_node and pins the rank's host threads next to its GPU (bench.py: pin_to_gpu_numa).
 * Returns 0, HP3D_ERR_HIP, or HP3D_ERR_UNSUPPORTED in the CPU interpreter build. */
int hp3d_device_pci_bus_id(int device, char* buf, int cap);

/* ---- context ----------------------------------------------------------------------------
 * replaces: tf.Session(config=...) + graph construction (run.py:44-50).                     */
int hp3d_create(int device, hp3d_ctx** out);
int hp3d_destroy(hp3d_ctx* ctx);
const char* hp3d_last_error(hp3d_ctx* ctx);          /* ctx may be NULL: last global error   */
void* hp3d_stream(hp3d_ctx* ctx);                    /* the hipStream_t all work is queued on */
int hp3d_sync(hp3d_ctx* ctx);
/* options: "empty_reduce" = "inf" | "fltmax" (oracle/general.py EMPTY_REDUCE);
 *          "mask_grow"    = "auto" (default) | "lds" | "global": the seeded mask growth on bit-packed maps in one workgroup's LDS
 *                            (mask_grow_kernel; "auto" takes it wherever its three maps fit, 3 * H * (ceil(W / 32) + 1) + 2 words
 *                            <= 159 KB, e.g. 640x640 or 480x864) or with the maps in global scratch (mask_grow_global_kernel: any
 *                            frame, e.g. 720x1280, 1080x1920; "auto" beyond the LDS size).  "lds" refuses larger frames
 *                            (HP3D_ERR_ARG "too large for the in-LDS mask growth"); "global" takes the scratch kernel at every size.
 *                            Both give the same results bit for bit;
 *          "conv_impl"    = "mfma" (default: direct MFMA kernel, and float32 Winograd F(2x2,3x3) for the stride-1 3x3
 *                            layers with Cout%64==0 and the 7x7 layers -- taken as nine 3x3 blocks -- whenever the grid
 *                            fills the chip, >= 256 work items) | "direct" (never Winograd: bit-identical to an fmaf
 *                            chain) | "winograd" (whenever the shape allows; per-op hp3d_conv2d then refuses other
 *                            shapes) | "naive" (debug cross-check kernel, never a fallback);
 *          "streams"      = "auto" (default) | "1" | "2": whole-path calls run the two halves of their batch concurrently
 *                            on two HIP streams (second arena, shared weights; fills the tail rounds of the persistent
 *                            kernels and the launch gaps).  auto = 2 when each half has at least 2.4 M input pixels (B = 32 at
 *                            480x640, two chunks of 32 at 240x320 / 320x320; 3 M until round 6) or, round 6, for 40 <= B < 64 in float32 mode (a full
 *                            chunk followed by a latency-bound remainder on one stream: B = 40 2487 -> 2616 images/s), else 1 (round 4: with "wino4_tail" the one-stream run no longer
 *                            loses a partial last round, and halves of 16 images fill the chip worse).  Results equal "1" to
 *                            rounding (images are independent; a half may take the small-batch kernel plan).  So within
 *                            32 < B < 64 (float32; auto = 2 from B = 40 at <= 320x320) an image's results depend on the call's
 *                            total B: to rounding, and through det pixels on the knife edge also in its mask / crop;
 *                            profiling / graph replay use one stream.  The halves overlap on the device-pointer entry points
 *                            (hp3d_infer_full_dev ...); with HOST output buffers the first half's pageable device->host
 *                            copies block the host before the second half is enqueued;
 *          "wino_splitk"  = "1" (default) | "0": Winograd layers whose work items under-fill the chip (small batches) split
 *                            their channel steps over up to 16 workgroups and sum float32 partials in a fixed order;
 *          "wino2"        = "auto" (default) | "0" | "1": which of the two float32 Winograd kernels a 3x3 / 7x7 layer takes when both
 *                            can run it.  conv_wino.hip gives one wave a whole SIMD (256 accumulators, 32-channel steps, 128-cout
 *                            items: long reductions); conv_wino2.hip runs two workgroups per CU on v_mfma_f32_16x16x4_f32 (128
 *                            accumulators, 16-channel steps, 64-cout items), so one item's epilogue / waits are the other's MFMA
 *                            time and a launch has four times as many, four times finer work items.  auto = a per-layer cost
 *                            model of both kernels' rounds of work items (engine.hip:wino2_auto): in practice conv_wino2 for
 *                            launches that under-fill or badly quantise conv_wino's grid (small batches), conv_wino for B = 32;
 *                            "1" = wherever the shape allows (tests); "0" = never.  Same arithmetic: results agree to
 *                            accumulation order;
 *          "wino4"        = "auto" (default) | "pose" | "0" | "1": Winograd F(4x4,3x3) (conv_wino4.hip: 36 products per 4x4 outputs, 2.25
 *                            multiply-adds per output instead of F(2x2,3x3)'s 4) for the 3x3 / 7x7 layers.  auto = every trunk layer a
 *                            per-layer cost model of the three Winograd kernels gives to it (filled launches: B >= 4 ... 8); "pose" =
 *                            PoseNet2D only (HandSegNet's score map feeds the mask threshold: with "auto" ~2 % more images differ from
 *                            the all-direct-kernel run in a mask pixel -- never in the crop box or, beyond 1e-4, in a keypoint over 512
 *                            images, scripts/mask_flip_rate.py); "1" = wherever the shape allows (tests); "0" = never.  Float32
 *                            throughout; end to end it moves heat-maps by 5e-6 and 3-D keypoints by 3e-6;
 *          "wino7"        = "auto" (default) | "0" | "1": PoseNet2D's ten 7x7 layers (ColorHandPose3DNetwork.py:206-215) as Winograd
 *                            F(4x4,4x4) over the filter's four 4x4-tap blocks (conv_wino7.hip, round 5: 169 instead of 289 plane products per
 *                            16 outputs, the transformed input shared by the four blocks, one work item = 16 tiles x 64 couts with no channel
 *                            split) when the launch fills the chip (>= 160 work items: B >= 20 on the 32 x 32 score maps) | never (the
 *                            nine-3x3-block form on conv_wino4.hip / conv_wino2.hip) | whenever the shape allows (tests).  Float32 throughout,
 *                            the same rounding error as the nine-block form (profiles/r05_wino7_numerics.md).  Launches below that fill
 *                            (small batches) run the same kernel with the 16-channel chunks split over workgroups -- raw 4x4 sums per
 *                            split, added in order by the reduce launch with bias and activation -- when "wino_splitk" = "1";
 *          "wino7_ksplit" = "auto" (default) | N: the number of channel splits of such a launch (auto: CUs / work items, at most one split
 *                            per chunk; N: tests and tuning, clamped to the number of chunks);
 *          "pw2"          = "1" (default) | "0" | "force": the 1x1 head pairs of both trunks (conv6_1 + conv6_2; conv5_1 + conv5_2, conv6_6 + conv6_7,
 *                            conv7_6 + conv7_7: ColorHandPose3DNetwork.py:160-161,202-203,213-214) as ONE launch each with the wide intermediate in
 *                            LDS (conv_pw2.hip, round 5) when the launch has a workgroup of 64 pixels per CU | two launches of the general kernel |
 *                            whenever the shapes allow (tests).  Float32 mode only;
 *          "wino4_tail"   = "1" (default) | "0": conv_wino4.hip deals its work items round-robin to one workgroup per CU; when the last
 *                            round is at most half full (HandSegNet's 40x40 layers at B = 32: 800 items on 256 CUs = 3.125 rounds) its
 *                            items run as channel slices -- one piece per CU, raw sums to a scratch of 2 pieces x CUs x 128 KB = 64 MiB per context on a 256-CU
 *                            MI355X (the second-stream child context grows its own), added in slice order by a small
 *                            reduce launch (deterministic; the summation order differs from the unsplit item: float32 rounding);
 *          "first_touch"  = "auto" (default) | "0" | "1": conv1_1's kernel is store-bound and gathers its operands one tile ahead; an input
 *                            image that is COLD in the memory system (the caller's device buffer, an upload -- not the crop or the uint8
 *                            front end's output, which the kernel in front has just written) costs it a third of its rate.  auto: such an
 *                            image of 8 ... 128 MB is streamed once through the memory-side cache first (13 us for 39 MB; HandSegNet's
 *                            conv1_1 at B = 32, 320 x 320: 0.253 -> 0.175 ms) | never | always.  Reads only: results unchanged;
 *          "first_touch_beside" = "1" (default) | "0": that read pass runs on a second stream beside conv1_1 | in front of it;
 *          "first_walk"   = "balanced" (default) | "rows": conv1_1's kernel (conv_first.hip) gives every resident workgroup one run of
 *                            consecutive 8 x 16 tiles, all runs within a tile of the same length | a whole tile row per workgroup (rounds 2-4;
 *                            kept for A/B timing).  Bit-identical results;
 *          "lift_overlap" = "1" (default) | "0": the unfused lifting stage (batches above 4) runs ViewpointNet on a second stream beside
 *                            PosePrior (the towers share only their input, ColorHandPose3DNetwork.py:231-235; 12 + 12 short dependent launches)
 *                            | one after the other.  Same kernels, same results bit for bit;
 *          "lift_fused"   = "auto" (default) | "0" | "1": PosePrior + ViewpointNet + the lifting epilogue
 *                            (ColorHandPose3DNetwork.py:221-334) as ONE persistent launch with grid barriers (lift_fused.hip)
 *                            instead of 24 launches.  auto = for at most 4 images per call (the stage is latency-bound there:
 *                            0.33 -> 0.14 ms at B = 1); "1" = always (tests; needs the whole grid resident, which the launcher
 *                            checks); "0" = never.  Results agree to accumulation order (2-5e-7);
 *          "micro_batch"  = "N" | "auto": whole-path calls (hp3d_infer_full*) run as consecutive chunks of at most N
 *                            images ("0" = never split; default "auto" = at most 32 in float32 mode -- fewer when H x W x 64 floats x N
 *                            would pass 2^31 bytes, e.g. 480x640: balanced chunks of <= 27 -- and no split with f16 trunks).
 *                            Bit-identical to making the calls chunk by chunk;
 *          "track_margin"  = "1.25" (default) | a number in (0, 16]: the factor hp3d_track_step* / hp3d_track_box put on the box size
 *                            the readers' rule gives ("1" = that rule bit for bit).  1.25 is what the detection path puts on its own box
 *                            (ColorHandPose3DNetwork.py:84): a policy choice for the hand's motion between frames, not a measurement;
 *          "track_min_score" = "off" (default) | a number: a tracked image counts as lost when its confidence is below it.  A useful
 *                            value depends on the trained weights: callers calibrate it on the confidence the steps return;
 *          "track_redetect" = "0" (default: never) | N: every N-th tracking step is a detect step that re-boxes every image
 *                            (hp3d_track_hands_step*: that fills free slots only, kept slots are not re-boxed);
 *          "track_partial_detect" = "0" (default) | "1": a detect step of hp3d_track_step / _dev / _u8 that only `lost` flags caused runs
 *                            HandSegNet, the soft-max and the mask growth on the lost frames only, at batch m = their number per chunk; see
 *                            "partial detection" below.  "0": every call enqueues what it did without the option.  Anything else:
 *                            HP3D_ERR_ARG.  hp3d_track_hands_step* and every hp3d_infer_* call IGNORE the option;
 *          "track_hands_partial_detect" = "0" (default) | "1": the same for hp3d_track_hands_step / _dev / _u8 / _nv12[_dev] / _px[_dev]: a detect
 *                            step that flags alone caused runs HandSegNet, the soft-max and the claimed multi-hand growth on the frames that
 *                            have a valid slot lost or no valid slot, at batch m = their number per chunk; see "partial detection, several
 *                            hands" below.  "0": every call enqueues what it did without the option.  Anything else: HP3D_ERR_ARG.
 *                            hp3d_infer_hands*, hp3d_track_step* and every hp3d_infer_* call IGNORE the option;
 *          "detect_scale" = "1" (default) | "2" ... "8", an integer f: the DETECT steps of hp3d_track_step* / hp3d_track_hands_step* find the
 *                            hand on the frame's f x f area mean ([ceil(H/f), ceil(W/f)], at least 16 x 16: HP3D_ERR_ARG before any launch
 *                            otherwise) and crop from the frame itself; see "detection on a reduced frame" below.  "1": detect on the
 *                            frame, every call enqueues what it did without the option.  Tracked steps are the same at every f.
 *                            hp3d_infer_full*, hp3d_infer_2d* and hp3d_infer_hands* IGNORE the option (their score-map and mask outputs
 *                            have the frame's size).  A change between two steps counts as a change of shape: the next step detects.
 *                            The default and which f still finds a hand are policy, not measurement;
 *          "nv12_matrix"  = "bt709" (default) | "bt601" | "bt709_full" | "bt601_full": the colour matrix of the NV12 entry points; see
 *                            "NV12 frames" below.  Anything else: HP3D_ERR_ARG.  Every other call ignores it;
 *          "hands_min_area" = "0" (default: off) | N: hp3d_infer_hands* / hp3d_masks_from_scoremap drop objects of fewer than N pixels
 *                            instead of reporting them as hands.  A useful value depends on the trained weights: callers calibrate it on
 *                            the `area` every call returns;
 *          "hands_compact" = "0" (default) | "1": hp3d_infer_hands* and hp3d_track_hands_step* run everything behind the boxes -- crop,
 *                            PoseNet2D, lifting, heat-map up-sampling, keypoint detection, the tracker's box rule -- on the slots that hold
 *                            a hand only (valid = 1), at batch m = their number per chunk, and return the absent-slot fill for the others;
 *                            see "compaction of absent hand slots" below.  "0": every call enqueues what it did without the option.  Anything
 *                            else: HP3D_ERR_ARG.  The single-hand entry points ignore it;
 *          "f16_impl"     = "h16" (default) | "mfma" | "h16_force": with half-precision trunks (hp3d_finalize_weights dtype 1),
 *                            the 3x3 / stride-1 layers with Cin >= 64 run on the half-precision trunk kernel (conv_h16.hip)
 *                            whenever their grid fills the chip | never (general kernel only) | whenever the shape allows
 *                            (tests).  Same MFMA and packed weights either way: results agree to accumulation order;
 *          "f16_k7k1"     = "1" (default) | "0": with "f16_impl" on conv_h16.hip, PoseNet2D's 7x7 score-map stages and the 1x1 layers with
 *                            >= 64 couts also run on it (single-buffer forms, patch of (16 + k - 1)^2 pixels) | on the general kernel.
 *                            Same MFMA and packed weights: results agree to accumulation order;
 *          "f16_fuse12"   = "1" (default) | "0" | "ring" | "resident": with half-precision trunks and the layer on conv_h16.hip, conv1_1 is computed
 *                            inside conv1_2's patch stage (one launch for conv1_1 + conv1_2 + max-pool; conv1_1's activation
 *                            never reaches HBM).  Bit-identical to the two-launch form.  Two forms of that launch (round 6): "ring" = two
 *                            workgroups per CU, conv1_2's filters through a register ring; "resident" = one workgroup per CU with the
 *                            filters resident in registers and the next tile's patch built between the MFMAs of the current one
 *                            (conv_h16_first_kernel); "1" takes "resident" from four tiles per CU on, else "ring";
 *          "wino4_split"  = "0" (default) | "auto" | "1" (round 6): the 3x3 / stride-1 trunk layers with Cin >= 128 whose launch fills the chip run
 *                            Winograd F(4x4,3x3) with the plane products on v_mfma_f32_16x16x32_bf16 over THREE bfloat16 pieces per operand (six
 *                            products, float32 accumulate: conv_wino4s.hip) | never | wherever the shape allows (tests).  Float32 in and out; per
 *                            layer as exact as "wino4" (0.7 ... 1.6x its error per shape, profiles/r06_split_numerics.md) and, when built, 1.03-1.09x its (since conv_wino4's late round-6 gains: 0.98x) speed:
 *                            an option, not the default;
 *          "fc_tail"      = "1" (default) | "0" (round 6): ViewpointNet's three FC layers (ColorHandPose3DNetwork.py:299-307) as two launches -- the K slices
 *                            of fc_vp0, then their fixed-order reduction + fc_vp1 + fc_vp_u in one -- | as three partial + reduce pairs.  Same sums up
 *                            to the order inside fc_vp1 (1e-7);
 *          "tiny_gemm"    = "1" (default) | "0" (round 6): ViewpointNet/conv_vp_2_2 (3x3 / stride 2 on the 8x8 map, 16 output pixels per image) as a split-K
 *                            GEMM over its output pixels with the HWIO filter as the matrix | on the general kernel's 8x8-pixel tiles;
 *          "kp_up_side"   = "1" (default) | "0" (round 6): with "lift_overlap", the whole-path calls' heat-map up-sampling runs behind ViewpointNet on the
 *                            second stream | behind PosePrior on the first.  Bit-identical;
 *          "graph"        = "0" | "1": the device-pointer entry points (hp3d_infer_full_dev, hp3d_posenet2d_dev) replay
 *                            their launch sequence as one hipGraph from the third identical call on (same shape and
 *                            pointers); meant for small batches.  Default "0".                               */
int hp3d_set_option(hp3d_ctx* ctx, const char* key, const char* value);

/* ---- weights ----------------------------------------------------------------------------
 * replaces: ColorHandPose3DNetwork.init / PosePriorNetwork.init, i.e. pickle dict ->
 * tf.contrib.framework.assign_from_values (nets/ColorHandPose3DNetwork.py:34-59,
 * nets/PosePriorNetwork.py:36-57).  `tf_var_name` is the pickle key, e.g.
 * "PoseNet2D/conv6_1/weights"; conv weights HWIO [k,k,Cin,Cout], FC weights [in,out],
 * biases [out] (utils/general.py:41-50,117-126).  Data is copied; unknown names are
 * rejected (HP3D_ERR_ARG), mis-shaped ones too.                                              */
int hp3d_set_weight(hp3d_ctx* ctx, const char* tf_var_name, const float* data,
                    const int64_t* shape, int rank);
/* Pack everything set so far for the device (repack HWIO -> MFMA fragment order, permute
 * the concat channels of conv6_1/conv7_1, upload).  Nets whose variables are all present
 * become runnable; a net with only some of its variables is an error.
 * dtype 0: float32 everywhere (exact f32 MFMA).  dtype 1 (BASELINE config 5): the HandSegNet / PoseNet2D
 * filters and activations are float16 on v_mfma_f32_32x32x16_f16 with float32 accumulation, biases and
 * score-map heads; the lifting nets, the mask stage and all outputs stay float32.                   */
int hp3d_finalize_weights(hp3d_ctx* ctx, int dtype);
/* The packed device blob (identical layout on every rank): size, export to / import from a
 * device buffer.  Used for the one-off RCCL broadcast of weights (bench.py, N>1).           */
int hp3d_weights_blob_bytes(hp3d_ctx* ctx, size_t* bytes);
int hp3d_weights_blob_export(hp3d_ctx* ctx, void* dev_dst);
int hp3d_weights_blob_import(hp3d_ctx* ctx, const void* dev_src, int nets_mask);
int hp3d_nets_mask(hp3d_ctx* ctx);   /* bit0 HandSegNet, bit1 PoseNet2D, bit2 PosePrior, bit3 ViewpointNet, bit4 bottleneck, bit5 f16 trunks */

/* ---- whole-path entry points ------------------------------------------------------------
 * hp3d_infer_full   replaces ColorHandPose3DNetwork.inference (nets/ColorHandPose3DNetwork.py:61-99)
 *   image [B,H,W,3] (x/255-0.5 done by the caller, run.py:59), hand_side [B,2] one-hot ->
 *   hand_scoremap [B,H,W,2], image_crop [B,256,256,3], scale_crop [B,1], center [B,2] (row,col),
 *   keypoints_scoremap [B,256,256,21], keypoint_coord3d [B,21,3].  Any H, W >= 16 (the VALID 2x2 max-pools floor odd
 *   extents and the logits are resized from floor(H/8) x floor(W/8) back to H x W, as in the reference) with
 *   H * W * 64 * 4 < 2^31, i.e. at most 8388607 pixels per image (2160x3840 is inside): one image's largest activation must fit
 *   the 32-bit offsets of the convolution kernels.  Larger frames -> HP3D_ERR_ARG before any launch.  The same holds for
 *   hp3d_infer_2d*, hp3d_infer_full_u8* (at the network size) and hp3d_handsegnet.
 * hp3d_infer_2d     replaces .inference2d (:101-129): keypoints_scoremap, image_crop, scale_crop, center.
 * hp3d_handsegnet   replaces .inference_detection (:131-168): scoremap_large [B,H,W,2]
 *   (scoremap_small [B,H/8,W/8,2] is the pre-upsampling map, for staged parity tests).
 * hp3d_posenet2d    replaces .inference_pose2d (:170-219): the 3 scoremaps [B,h/8,w/8,21].
 * hp3d_poseprior    replaces PosePriorNetwork(variant).inference (nets/PosePriorNetwork.py:59-95):
 *   scoremap256 [B,256,256,21] -> coord_xyz_rel_normed [B,21,3], coord3d [B,21,3], R [B,3,3]
 *   (R untouched for direct/bottleneck/local, where the reference returns None).
 * hp3d_pose3d       replaces ._inference_pose3d (:221-247) on a [B,32,32,21] scoremap.
 * hand_mask (extra, may be NULL): the internal objectmap [B,H,W] of single_obj_scoremap
 *   (utils/general.py:233-268), exposed so tests can assert mask equality first.            */
int hp3d_infer_full(hp3d_ctx* ctx, int B, int H, int W, const float* image, const float* hand_side,
                    float* hand_scoremap, float* image_crop, float* scale_crop, float* center,
                    float* keypoints_scoremap, float* keypoint_coord3d, float* hand_mask);
int hp3d_infer_full_dev(hp3d_ctx* ctx, int B, int H, int W, const float* image, const float* hand_side,
                        float* hand_scoremap, float* image_crop, float* scale_crop, float* center,
                        float* keypoints_scoremap, float* keypoint_coord3d, float* hand_mask);
/* The same calls with the host post-processing of the scripts done on the device (run.py:72-73, eval2d.py:93-94,
 * eval2d_gt_cropped.py:76): keypoint_hw_crop [B,21,2] int32 = detect_keypoints(keypoints_scoremap[b])
 * (utils/general.py:331-344: per channel the first maximum, (row, col)) and keypoint_hw [B,21,2] float64 =
 * trafo_coords(keypoint_hw_crop, center, scale_crop, 256) (utils/general.py:347-357).  Computed from the 32x32 maps
 * by re-evaluating tf.image.resize_images' arithmetic, so keypoints_scoremap (5.5 MB / image) may be NULL: eval loops
 * need no heat-map copy.  Bit-exact with the reference functions applied to the up-sampled map, ties included.      */
int hp3d_infer_full_kp(hp3d_ctx* ctx, int B, int H, int W, const float* image, const float* hand_side,
                       float* hand_scoremap, float* image_crop, float* scale_crop, float* center,
                       float* keypoints_scoremap, float* keypoint_coord3d, float* hand_mask,
                       int32_t* keypoint_hw_crop, double* keypoint_hw);
int hp3d_infer_full_kp_dev(hp3d_ctx* ctx, int B, int H, int W, const float* image, const float* hand_side,
                           float* hand_scoremap, float* image_crop, float* scale_crop, float* center,
                           float* keypoints_scoremap, float* keypoint_coord3d, float* hand_mask,
                           int32_t* keypoint_hw_crop, double* keypoint_hw);
int hp3d_infer_full_kp_u8(hp3d_ctx* ctx, int B, int Hin, int Win, const uint8_t* image_u8, int H, int W,
                          const float* hand_side, float* hand_scoremap, float* image_crop, float* scale_crop,
                          float* center, float* keypoints_scoremap, float* keypoint_coord3d, float* hand_mask,
                          int32_t* keypoint_hw_crop, double* keypoint_hw);
/* SURVEY.md 8f N2 -- the step immediately before the hot path, on device: uint8 frames
 * [B,Hin,Win,3] -> x/255-0.5 (data/BinaryDbReader.py:182, run.py:59) -> tf.image.resize_images to H x W
 * (eval_full.py:50, eval2d.py:53; equal sizes = identity) -> hp3d_infer_full.  4x less H2D traffic.      */
int hp3d_infer_full_u8(hp3d_ctx* ctx, int B, int Hin, int Win, const uint8_t* image_u8, int H, int W,
                       const float* hand_side, float* hand_scoremap, float* image_crop, float* scale_crop,
                       float* center, float* keypoints_scoremap, float* keypoint_coord3d, float* hand_mask);
int hp3d_preprocess_u8(hp3d_ctx* ctx, const uint8_t* image_u8, int B, int Hin, int Win, int H, int W, float* out);
int hp3d_infer_2d(hp3d_ctx* ctx, int B, int H, int W, const float* image,
                  float* keypoints_scoremap, float* image_crop, float* scale_crop, float* center);
int hp3d_infer_2d_kp(hp3d_ctx* ctx, int B, int H, int W, const float* image, float* keypoints_scoremap,
                     float* image_crop, float* scale_crop, float* center,
                     int32_t* keypoint_hw_crop, double* keypoint_hw);   /* + detect_keypoints / trafo_coords, as above */
int hp3d_handsegnet(hp3d_ctx* ctx, int B, int H, int W, const float* image,
                    float* scoremap_large, float* scoremap_small);
int hp3d_posenet2d(hp3d_ctx* ctx, int B, int H, int W, const float* image_crop,
                   float* scoremap0, float* scoremap1, float* scoremap2);
int hp3d_posenet2d_dev(hp3d_ctx* ctx, int B, int H, int W, const float* image_crop,
                       float* scoremap0, float* scoremap1, float* scoremap2);
int hp3d_poseprior(hp3d_ctx* ctx, int B, int variant, const float* scoremap256, const float* hand_side,
                   float* coord_xyz_rel_normed, float* coord3d, float* rot_mat);
int hp3d_pose3d(hp3d_ctx* ctx, int B, const float* scoremap32, const float* hand_side,
                float* coord_xyz_rel_normed, float* coord_can, float* rot_mat);

/* ---- tracking: a hand across video frames -------------------------------------
 * The whole-path calls above treat every frame as a single picture (ColorHandPose3DNetwork.inference, :61-99): HandSegNet over the
 * whole frame, mask, box, crop, then PoseNet2D and the lifting stage.  On frame t + 1 of a video the 21 keypoints of frame t already
 * say where the hand is.  A tracking step crops with the box the dataset readers' hand_crop rule derives from keypoints
 * (data/BinaryDbReader.py:268-308, data/BinaryDbReaderSTB.py:219-259 -- the crops PoseNet2D was trained on and
 * eval2d_gt_cropped.py evaluates it on): centre = keypoint 12, size = 2 x the largest distance from the centre to the keypoints'
 * bounding box, x option "track_margin", clamped to [50, 500], scale = 256 / size clamped to [1, 10] -- applied to the PREVIOUS
 * step's predicted keypoints, and runs no HandSegNet, soft-max or mask growth ("tracked step").  A "detect step" runs them for the
 * whole batch as hp3d_infer_full does and then, per image, keeps the tracked box where the previous step did not flag it as lost.
 * A step detects: the first time after hp3d_create / hp3d_track_reset / a change of (B, H, W); when the previous step flagged ANY
 * image as lost (the whole batch detects: one kernel plan per step, no gather -- unless option "track_partial_detect"); and, with
 * option "track_redetect" = N > 0, every N-th step (a scheduled re-detection takes HandSegNet's box for every image).  The decision
 * is taken on the host from the previous step's flags before anything is enqueued; a tracked step needs no HandSegNet weights.
 * hp3d_track_reset    the next step detects.
 * hp3d_track_seed     start from boxes the caller has (another detector, ground truth): center [B,2] (row, col) finite, scale [B] > 0;
 *                     the next step for (B, H, W) is a tracked step.
 * hp3d_track_step     image [B,H,W,3] (x/255-0.5 done by the caller), hand_side [B,2] -> image_crop [B,256,256,3], scale_crop [B,1] and
 *                     center [B,2] (the boxes THIS step cropped with), keypoints_scoremap [B,256,256,21] (may be NULL like any output),
 *                     keypoint_coord3d [B,21,3], keypoint_hw_crop [B,21,2] int32 and keypoint_hw [B,21,2] float64 (detect_keypoints /
 *                     trafo_coords as in hp3d_infer_full_kp), confidence [B] = the mean over the 21 channels of the maximum of
 *                     PoseNet2D's last 32x32 score map, lost [B] int32 = 1 where the NEXT box is unusable (keypoint 12 not finite or
 *                     outside the frame: row < 0, row > H, col < 0, col > W; or confidence below option "track_min_score"),
 *                     detected [B] int32 = 1 where this step's box came from HandSegNet.  hand_scoremap / hand_mask are not outputs.
 * hp3d_track_step_dev the same on device pointers, stream-ordered; the flags also travel to a page-locked buffer of the context and
 *                     the next step waits for that copy before it decides -- the only wait tracking adds.
 * hp3d_track_step_u8  uint8 frames [B,Hin,Win,3] on the host; Hin x Win must equal H x W (HP3D_ERR_UNSUPPORTED otherwise): a tracked
 *                     step crops straight from the uint8 frame and never builds the normalised float frame; a detect step
 *                     normalises it first as hp3d_infer_full_u8 does.
 * Batches above the micro-batch limit run chunk by chunk on one stream; half-precision trunks work; no graph replay.
 * hp3d_track_box (per-op) the box rule alone: keypoint_hw [B,21,2] float64 (row, col), score32 [B,32,32,21] or NULL (confidence 0,
 *                     no threshold test), margin = the factor on the size (0: option "track_margin") -> center [B,2], scale [B],
 *                     confidence [B], lost [B]; uses option "track_min_score"; with margin = 1 it is the readers' rule bit for bit.
 * hp3d_crop_and_resize_u8 (per-op) crop_image_from_xy (utils/general.py:163-196) straight from uint8 frames [B,H,W,3]: every tap is
 *                     normalised (x/255-0.5, data/BinaryDbReader.py:182) and interpolated; bit-identical to hp3d_preprocess_u8 at
 *                     equal sizes followed by hp3d_crop_and_resize.                                                           */
int hp3d_track_reset(hp3d_ctx* ctx);
int hp3d_track_seed(hp3d_ctx* ctx, int B, int H, int W, const float* center, const float* scale);
int hp3d_track_step(hp3d_ctx* ctx, int B, int H, int W, const float* image, const float* hand_side, float* image_crop,
                    float* scale_crop, float* center, float* keypoints_scoremap, float* keypoint_coord3d,
                    int32_t* keypoint_hw_crop, double* keypoint_hw, float* confidence, int32_t* lost, int32_t* detected);
int hp3d_track_step_dev(hp3d_ctx* ctx, int B, int H, int W, const float* image, const float* hand_side, float* image_crop,
                        float* scale_crop, float* center, float* keypoints_scoremap, float* keypoint_coord3d,
                        int32_t* keypoint_hw_crop, double* keypoint_hw, float* confidence, int32_t* lost, int32_t* detected);
int hp3d_track_step_u8(hp3d_ctx* ctx, int B, int Hin, int Win, const uint8_t* image_u8, int H, int W, const float* hand_side,
                       float* image_crop, float* scale_crop, float* center, float* keypoints_scoremap, float* keypoint_coord3d,
                       int32_t* keypoint_hw_crop, double* keypoint_hw, float* confidence, int32_t* lost, int32_t* detected);
int hp3d_track_box(hp3d_ctx* ctx, int B, int H, int W, const double* keypoint_hw, const float* score32, float margin, float* center,
                   float* scale, float* confidence, int32_t* lost);
int hp3d_crop_and_resize_u8(hp3d_ctx* ctx, const uint8_t* image_u8, int B, int H, int W, const float* center,
                            const float* scale, int crop_size, float* out);

/* ---- detection on a reduced frame (option "detect_scale" = f > 1) ----------------
 * A detect step of hp3d_track_step* / hp3d_track_hands_step* then runs, all in float32 op by op:
 *  1. the detection frame [Hd, Wd] = [ceil(H/f), ceil(W/f)]: pixel (y, x, c) = the mean of the frame's rows [y f, min((y+1) f, H)) x
 *     columns [x f, min((x+1) f, W)) (clipped windows, n = the real count).  float32 frames: the window added in row-major order as a
 *     sequential float32 sum, / float(n).  uint8 frames (hp3d_*_step_u8): the exact integer sum, (float(sum) / float(n)) / 255 - 0.5;
 *     the normalised full-size frame is never built (no preprocess_u8 launch);
 *  2. HandSegNet, the soft-max and the mask growth at (Hd, Wd) exactly as on a frame of that size; `area`, option "hands_min_area" and
 *     the growth cap are in detection-frame pixels;
 *  3. every box the growth wrote (fall-back boxes and absent slots included) to the frame: centre = centre_d * f + (f - 1) / 2,
 *     crop_size = crop_size_d * f, scale = clip(256 / (crop_size * 1.25), 0.25, 5);
 *  4. (multi-hand) before the growth, the kept slots to the detection frame for the claim rule: centre_d = (centre - (f - 1) / 2) / f,
 *     scale_d = scale * f;
 *  5. the per-image / per-slot choice, the crop -- from the FULL frame (hp3d_*_step_u8: straight from the uint8 frame, counted in
 *     "crop_u8_launches") -- and everything behind it in frame coordinates as without the option.
 * The activation arena and the micro-batch limit follow (Hd, Wd).  Profile rows "downscale" / "downscale_u8", "box_to_frame",
 * "box_to_detect"; counter "detect_scale_steps".  The per-op forms (host pointers, f in 1 ... 8):
 * hp3d_downscale / hp3d_downscale_u8  image [B,H,W,3] float32 / uint8 -> out [B,ceil(H/f),ceil(W/f),3] (rule 1)
 * hp3d_boxes_to_frame   center_d [n,2], crop_size_d [n] -> center [n,2], crop_size [n], scale [n] (rule 3)
 * hp3d_boxes_to_detect  center [n,2], scale [n] -> center_d [n,2], scale_d [n] (rule 4)                                          */
int hp3d_downscale(hp3d_ctx* ctx, const float* image, int B, int H, int W, int f, float* out);
int hp3d_downscale_u8(hp3d_ctx* ctx, const uint8_t* image_u8, int B, int H, int W, int f, float* out);
int hp3d_boxes_to_frame(hp3d_ctx* ctx, int n, int f, const float* center_d, const float* crop_size_d, float* center, float* crop_size,
                        float* scale);
int hp3d_boxes_to_detect(hp3d_ctx* ctx, int n, int f, const float* center, const float* scale, float* center_d, float* scale_d);

/* ---- partial detection (option "track_partial_detect" = "1") --------------------
 * hp3d_track_step / _dev / _u8 only.  Which steps detect is unchanged; a fresh step and a scheduled one (option "track_redetect") re-box
 * every image and run as without the option.  In a detect step that only `lost` flags caused, per chunk of nb frames (the micro-batch
 * limit stays), with L = the chunk's frames whose previous `lost` flag is set, ascending, m = |L|:
 *  - m = nb: the chunk runs as without the option (same launches, same bits).
 *  - m = 0 (another chunk holds the lost frame): the chunk is enqueued as a tracked chunk -- no HandSegNet, soft-max or mask growth,
 *    hp3d_track_step_u8 crops straight from the uint8 frame -- and detected = 0.
 *  - 0 < m < nb: HandSegNet, the soft-max and the mask growth run at batch m on the frames of L; crop, PoseNet2D, lifting, keypoint
 *    detection and the box rule run at batch nb as always.  A frame of L gets the box the same ops give on a batch made of those m
 *    frames -- at "detect_scale" = 1 hp3d_infer_full's center / scale_crop on the gathered frames bit for bit, at f > 1 the chain
 *    hp3d_downscale[_u8] -> hp3d_handsegnet -> hp3d_mask_from_scoremap -> hp3d_boxes_to_frame on them -- and detected = 1.  Any other
 *    frame keeps its tracked box bit for bit, detected = 0, and EVERY output of it is bit-equal to the same step with the option off.
 *    The frames of L agree with the option-off step to the end-to-end tolerances only: HandSegNet's kernel plan follows m.
 *    hp3d_track_step_u8 at f = 1 normalises the m frames only and crops all nb straight from the uint8 frame (counted in
 *    "crop_u8_launches"; bit-identical to normalise-then-crop); at f > 1 only the m detection frames are built.
 * The step is a detect step like any other: it needs HandSegNet weights, counts once in "track_detect_steps" (and "detect_scale_steps"),
 * and the schedule of "track_redetect" restarts.  The lists L / positions are built on the device from the flags the previous step left
 * there; the host learns m from its own copy of the same flags: no wait is added and nothing is read back.
 * Profile rows "track_partial_index", "frame_gather", "preprocess_u8_idx", "downscale_idx" / "downscale_u8_idx", "track_select_pos";
 * counters "track_partial_frames_run" / "track_partial_frames_skipped" / "frame_gather_launches".  The per-op form (host pointers):
 * hp3d_gather_frames  exactly one of image [B,H,W,3] float32 / image_u8 [B,H,W,3]; f in 1 ... 8; idx [m] strictly ascending in [0, B),
 *                     1 <= m <= B -> out [m,ceil(H/f),ceil(W/f),3]: bit for bit what hp3d_downscale / hp3d_downscale_u8 (f > 1),
 *                     hp3d_preprocess_u8 at equal sizes (uint8, f = 1) or a plain copy (float32, f = 1) give on the gathered frames.
 *                     Anything else: HP3D_ERR_ARG before any launch.                                                              */
int hp3d_gather_frames(hp3d_ctx* ctx, const float* image, const uint8_t* image_u8, int B, int H, int W, int f, const int32_t* idx, int m,
                       float* out);

/* ---- partial detection, several hands (option "track_hands_partial_detect" = "1") ----
 * hp3d_track_hands_step / _dev / _u8 / _nv12[_dev] / _px[_dev] only ("tracking several hands per frame" below).  Which steps detect is
 * unchanged.  A fresh step runs whole (there is nothing to keep) and so does a scheduled one (option "track_redetect": it is how a hand
 * that enters any picture is found).  Only a detect step that flags alone caused -- a valid slot lost, or an image with no valid slot --
 * can be partial.  Per chunk of nb frames (at most micro_batch / K, as always), with L = the chunk's frames that have a valid slot
 * flagged lost or no valid slot at all, ascending, m = |L|:
 *  - m = nb: the chunk runs as without the option (same launches, same bits).
 *  - m = 0 (another chunk holds the loss): the chunk is enqueued as a tracked chunk -- no HandSegNet, soft-max or growth; detected = area
 *    = claimed = 0.
 *  - 0 < m < nb: the m frames go dense to HandSegNet (as under "track_partial_detect": a copy, the normalisation of a uint8 / NV12 frame,
 *    or at "detect_scale" = f > 1 the indexed area mean); keep, box centre and box scale of their m K slots go dense; at f > 1 those
 *    boxes go to the detection frame; HandSegNet, the soft-max and the claimed multi-hand growth run at batch m; at f > 1 the boxes come
 *    back to the frame; then one select writes all nb K slots, the crop of all nb K slots is taken from the full frame (a uint8 / NV12
 *    frame: straight from it) and PoseNet2D, lifting, keypoint detection and the box rule run at batch nb K as always.
 * What is guaranteed:
 *  - A frame of L gets, bit for bit, what hp3d_masks_from_scoremap_keep gives on hp3d_handsegnet of a batch made of those m frames with
 *    their own keep flags and boxes (at f > 1: hp3d_downscale* -> hp3d_handsegnet -> hp3d_boxes_to_detect -> hp3d_masks_from_scoremap_keep
 *    -> hp3d_boxes_to_frame), and then the per-slot choice of a detect step: a kept slot holds its tracked box, the others take the
 *    growth's; `claimed` is the growth's.  It agrees with the option-off step to the end-to-end tolerances only: HandSegNet's kernel
 *    plan follows m.
 *  - A kept slot of a frame outside L holds its tracked box, valid = 1, detected = area = claimed = 0, and every output of it but
 *    `claimed` is bit-equal to the same step with the option off (without "hands_compact": the back half runs at nb K either way).
 *  - An ABSENT slot of a frame outside L stays absent: the fall-back box, valid = 0, detected = area = claimed = 0.  THE ONE POLICY
 *    DIFFERENCE: the whole-batch step looks at that frame too and may put a newly found object into the slot (and counts in `claimed`
 *    the objects the frame's kept slots claim); the partial step does not look at that frame.  A hand that enters such a frame is found
 *    by the next scheduled or whole detect step -- callers who need it soon set "track_redetect".
 * The step is a detect step like any other: HandSegNet weights, one count in "track_hands_detect_steps" (and "detect_scale_steps"), the
 * schedule of "track_redetect" restarts.  The lists are built on the device from the flags the previous step left there; the host
 * learns m from its own copy of the same flags: no wait is added and nothing is read back.  With "hands_compact" = "1" the compacted back
 * half runs behind the select exactly as behind a whole chunk's (its one wait per detecting chunk included); a chunk with m = 0 takes its
 * flags from the host like a tracked step's.
 * Profile rows "track_hands_partial_index", "track_hands_slot_gather", "track_hands_select_pos" (and "frame_gather" / "preprocess_u8_idx"
 * / "preprocess_nv12_idx" / "downscale_idx" / "downscale_u8_idx" / "downscale_nv12_idx"); counters "track_hands_partial_frames_run" /
 * "track_hands_partial_frames_skipped" (frames of partial chunks) and "frame_gather_launches".  The per-op forms (host pointers):
 * hp3d_track_hands_partial_index  valid [nb,K], lost [nb,K] int32 -> idx [nb] (the frames of L ascending, then -1), pos [nb] (a frame's
 *                     index in L or -1), *m = |L| as the device counted it.
 * hp3d_track_hands_select_pos     pos [nb] in -1 ... m-1, keep [nb,K], the growth's dense results det_center [m,K,2] / det_scale /
 *                     det_valid / det_area / det_claimed [m,K] (may be NULL when m = 0) -> box_center [nb,K,2], box_scale [nb,K], valid
 *                     [nb,K] (all three are read first: a slot that keeps its own gets it back untouched), detected, area, claimed
 *                     [nb,K].                                                                                                   */
int hp3d_track_hands_partial_index(hp3d_ctx* ctx, int nb, int K, const int32_t* valid, const int32_t* lost, int32_t* idx, int32_t* pos,
                                   int32_t* m);
int hp3d_track_hands_select_pos(hp3d_ctx* ctx, int nb, int K, int m, const int32_t* pos, const int32_t* keep, const float* det_center,
                                const float* det_scale, const int32_t* det_valid, const int32_t* det_area, const int32_t* det_claimed,
                                float* box_center, float* box_scale, int32_t* valid, int32_t* detected, int32_t* area, int32_t* claimed);

/* ---- compaction of absent hand slots (option "hands_compact" = "1") -------------
 * Per chunk of frames (at most micro_batch / K), idx[0 .. m) = the slots b K + j with valid = 1, ascending: the state's flags on a tracked
 * step, what the per-slot choice wrote on a detect step, what the multi-hand growth wrote in hp3d_infer_hands* (a slot 0 over an empty
 * detection map has valid = 0 and does not run).
 *  - A valid slot idx[i] returns what the same ops give at batch m on frame idx[i] / K, the slot's box and its hand_side: the launches
 *    are those of any batch of m crops (the kernel plan follows m, so results agree with the option off to the end-to-end tolerances,
 *    not bit for bit; the crop, centre and scale are bit-equal).
 *  - An absent slot returns image_crop = kp_scoremap = coord3d = keypoint_hw = 0, keypoint_hw_crop = 0, confidence = 0, lost = detected =
 *    area = 0 (a policy: the fill values); center / scale_crop stay its fall-back box, and the tracker's state machine is unchanged (the
 *    slot holds that box with lost = 0).  The only difference to the option off: its confidence is 0, not the fall-back crop's score.
 *  - hand_scoremap, hand_mask, valid, area (hp3d_infer_hands*) and claimed are what they are with the option off.
 *  - A chunk without an absent slot takes the uncompacted path (same launches, same bits); a chunk without a hand enqueues nothing behind
 *    the boxes but the fill.
 * THE WAIT: on detect steps and in hp3d_infer_hands* the flags exist on the device only, so each chunk copies them to the host and waits
 * for the stream once (counter "hands_compact_waits") behind its HandSegNet pass -- also on the _dev entry points, which otherwise return
 * without waiting.  Tracked steps add no stream synchronise: the state's flags are on the host already.  (The idx / pos upload uses two
 * page-locked buffers in turn; before one is rewritten the host waits for the event behind its last upload -- two compacted chunks ago,
 * so it can hold the host only in a call of three or more compacted chunks -- and once more when the slot count grows.  Neither is
 * counted in "hands_compact_waits".)
 * Profile rows "slot_gather", "crop_and_resize_idx" / "crop_and_resize_idx_u8", "slot_scatter"; counters "hands_compact_slots_run" /
 * "hands_compact_slots_skipped" / "hands_compact_waits".  The per-op forms (host pointers):
 * hp3d_crop_and_resize_idx  exactly one of image [B,H,W,3] float32 / image_u8 [B,H,W,3]; center [B K,2], scale [B K]; idx [m] slot indices
 *                           -> out [m,crop_size,crop_size,3]: crop i = box idx[i] cut from image idx[i] / K (= hp3d_crop_and_resize /
 *                           hp3d_crop_and_resize_u8 on the gathered frames and boxes, bit for bit)
 * hp3d_slot_scatter         dense [m,words] (4-byte words), pos [ns] (dense index or -1) -> out [ns,words]: out[s] = dense[pos[s]], 0 where
 *                           pos[s] = -1.  `out` holds ns words + 4 floats and is read first: what lies behind the last slot must come
 *                           back untouched.  skew_words in 0 ... 3 shifts the device destination off its 16-byte alignment (the kernel
 *                           then takes its 4-byte form).                                                                                  */
int hp3d_crop_and_resize_idx(hp3d_ctx* ctx, const float* image, const uint8_t* image_u8, int B, int H, int W, int K, const float* center,
                             const float* scale, const int32_t* idx, int m, int crop_size, float* out);
int hp3d_slot_scatter(hp3d_ctx* ctx, const float* dense, const int32_t* pos, int ns, int m, int words, int skew_words, float* out);

/* ---- several hands per frame --------------------------------------------------
 * The whole-path calls above keep ONE object of HandSegNet's detection map per image: the one that grows from the arg-max of the
 * foreground score (single_obj_scoremap, utils/general.py:233-268).  These calls return up to K of them, 1 <= K <= HP3D_MAX_HANDS, from
 * one HandSegNet pass.  With R = the detection map: the next object grows (21x21 dilation inside R, the reference's pass cap) from the
 * first arg-max of the foreground score over R and is then removed from R, so objects are pairwise disjoint; an object of at least
 * option "hands_min_area" pixels becomes the next hand; at most 4 K objects are grown per image.  Hands come in the order of discovery
 * (descending peak score, ties to the first pixel in row-major order).  Slot 0 with "hands_min_area" off is hp3d_infer_full's hand bit for
 * bit; where the detection map is empty it keeps that call's fall-back box and reports valid = 0.  Slots left over: valid = 0, area = 0,
 * zero mask, the fall-back box of option "empty_reduce".  Per hand, centre / crop size / scale as hp3d_infer_full computes them.  An object
 * the pass cap cuts short leaves its remainder in R, which can come back as a later hand.
 * All B * K slots run through PoseNet2D and the lifting stage, absent ones on their fall-back crop (no compaction unless option "hands_compact": one kernel plan per
 * call, no host wait); slot j of image b is index b * K + j of every per-hand output.
 * hp3d_infer_hands      image [B,H,W,3], hand_side [B,K,2] (per slot: which hand is left or right is the caller's knowledge) ->
 *                       hand_scoremap [B,H,W,2], image_crop [B,K,256,256,3], scale_crop [B,K], center [B,K,2],
 *                       keypoints_scoremap [B,K,256,256,21], keypoint_coord3d [B,K,21,3], hand_mask [B,K,H,W],
 *                       keypoint_hw_crop [B,K,21,2] int32, keypoint_hw [B,K,21,2] float64 (as hp3d_infer_full_kp),
 *                       valid [B,K] int32, area [B,K] int32 (pixels of the hand's mask).  Any output may be NULL.
 * hp3d_infer_hands_dev  the same on device pointers, stream-ordered.
 * hp3d_infer_hands_u8   uint8 frames [B,Hin,Win,3] on the host, normalised and resized to H x W on the device as hp3d_infer_full_kp_u8.
 * Batches run in chunks of at most micro_batch / K frames on one stream; half-precision trunks work; no graph replay, no second stream.
 * K outside 1 ... HP3D_MAX_HANDS or a NULL hand_side -> HP3D_ERR_ARG before any launch.                                          */
#define HP3D_MAX_HANDS 4
int hp3d_infer_hands(hp3d_ctx* ctx, int B, int H, int W, int K, const float* image, const float* hand_side, float* hand_scoremap,
                     float* image_crop, float* scale_crop, float* center, float* keypoints_scoremap, float* keypoint_coord3d,
                     float* hand_mask, int32_t* keypoint_hw_crop, double* keypoint_hw, int32_t* valid, int32_t* area);
int hp3d_infer_hands_dev(hp3d_ctx* ctx, int B, int H, int W, int K, const float* image, const float* hand_side, float* hand_scoremap,
                         float* image_crop, float* scale_crop, float* center, float* keypoints_scoremap, float* keypoint_coord3d,
                         float* hand_mask, int32_t* keypoint_hw_crop, double* keypoint_hw, int32_t* valid, int32_t* area);
int hp3d_infer_hands_u8(hp3d_ctx* ctx, int B, int Hin, int Win, const uint8_t* image_u8, int H, int W, int K, const float* hand_side,
                        float* hand_scoremap, float* image_crop, float* scale_crop, float* center, float* keypoints_scoremap,
                        float* keypoint_coord3d, float* hand_mask, int32_t* keypoint_hw_crop, double* keypoint_hw, int32_t* valid,
                        int32_t* area);

/* ---- tracking several hands per frame -----------------------------------------
 * K slots per frame, 1 <= K <= HP3D_MAX_HANDS; every per-hand array is [B,K,...] at index b * K + j.  A slot follows its hand for as
 * long as it is not lost, so the slot index is the hand's identity from frame to frame.  The state is separate from hp3d_track_step*'s.
 * A step is a DETECT step -- the first one after hp3d_create / hp3d_track_hands_reset / a change of (B, K, H, W); when the previous step
 * flagged a valid slot as lost; when some image has no valid slot; with option "track_redetect" = N > 0 every N-th step -- or a TRACKED
 * step (no HandSegNet, no soft-max, no mask growth, no HandSegNet weights needed): the K crops of a frame come from the state's boxes.
 * The whole batch detects together.  On a detect step the slots that are valid and not lost are KEPT: they crop with their tracked box
 * (detected = 0), also on a scheduled re-detection.  The objects of the detection map are found as hp3d_infer_hands finds them; an
 * object is CLAIMED by a kept slot with box (c, s), half = 128 / s, when its bounding-box centre o has |o.row - c.row| <= half and
 * |o.col - c.col| <= half, or when c lies inside its bounding box (float32; a comparison with a NaN is false).  A claimed object is that
 * slot's hand found again: it is dropped (never tested against "hands_min_area") and counted for the lowest slot that claims it.  The
 * others fill the free slots in the order of discovery, lowest free slot first (detected = valid = 1, box and area as hp3d_infer_hands
 * gives them); free slots left over are absent (valid = 0, area = 0, the fall-back box of option "empty_reduce").  Every growth, claimed
 * or not, counts toward the cap of 4 K growths per image.  Absent slots run the back half on their fall-back crop (unless option "hands_compact"); their confidence is
 * reported, their lost flag is 0, and they keep that box until a detect step fills them.
 * hp3d_track_hands_reset   the next step detects and keeps nothing.
 * hp3d_track_hands_seed    center [B,K,2] (row, col), scale [B,K], valid int32 [B,K]: valid slots need a finite centre and a finite
 *                          scale > 0, every image at least one valid slot (HP3D_ERR_ARG otherwise); the next step at (B, K, H, W) is a
 *                          tracked one.
 * hp3d_track_hands_step    as hp3d_track_step with hand_side [B,K,2] and every output per slot, plus valid int32 [B,K], area int32 [B,K]
 *                          (the object's pixel count where detected = 1, else 0) and claimed int32 [B,K] (objects the slot claimed on
 *                          this step; 0 on a tracked step).  For a valid slot the next box, confidence and lost are hp3d_track_box's.
 * hp3d_track_hands_step_dev / _u8   as hp3d_track_step_dev / hp3d_track_step_u8.
 * hp3d_track_hands_box (per-op) hp3d_track_box per slot with valid gating: keypoint_hw [B,K,21,2], score32 [B,K,32,32,21] or NULL,
 *                          valid [B,K], the boxes the slots cropped with box_center [B,K,2] / box_scale [B,K] -> center, scale,
 *                          confidence, lost: hp3d_track_box's for a valid slot; an absent one holds its box with lost = 0.
 * Outputs may be NULL as for hp3d_track_step.  K outside 1 ... HP3D_MAX_HANDS or a NULL image / hand_side -> HP3D_ERR_ARG before any
 * launch.  Options "track_margin", "track_min_score", "track_redetect", "hands_min_area", "mask_grow", "empty_reduce" apply; batches
 * run in chunks of at most micro_batch / K frames on one stream; no graph replay.                                                  */
int hp3d_track_hands_reset(hp3d_ctx* ctx);
int hp3d_track_hands_seed(hp3d_ctx* ctx, int B, int H, int W, int K, const float* center, const float* scale, const int32_t* valid);
int hp3d_track_hands_step(hp3d_ctx* ctx, int B, int H, int W, int K, const float* image, const float* hand_side, float* image_crop,
                          float* scale_crop, float* center, float* keypoints_scoremap, float* keypoint_coord3d, int32_t* keypoint_hw_crop,
                          double* keypoint_hw, float* confidence, int32_t* lost, int32_t* detected, int32_t* valid, int32_t* area,
                          int32_t* claimed);
int hp3d_track_hands_step_dev(hp3d_ctx* ctx, int B, int H, int W, int K, const float* image, const float* hand_side, float* image_crop,
                              float* scale_crop, float* center, float* keypoints_scoremap, float* keypoint_coord3d,
                              int32_t* keypoint_hw_crop, double* keypoint_hw, float* confidence, int32_t* lost, int32_t* detected,
                              int32_t* valid, int32_t* area, int32_t* claimed);
int hp3d_track_hands_step_u8(hp3d_ctx* ctx, int B, int Hin, int Win, const uint8_t* image_u8, int H, int W, int K, const float* hand_side,
                             float* image_crop, float* scale_crop, float* center, float* keypoints_scoremap, float* keypoint_coord3d,
                             int32_t* keypoint_hw_crop, double* keypoint_hw, float* confidence, int32_t* lost, int32_t* detected,
                             int32_t* valid, int32_t* area, int32_t* claimed);
int hp3d_track_hands_box(hp3d_ctx* ctx, int B, int K, int H, int W, const double* keypoint_hw, const float* score32, float margin,
                         const int32_t* valid, const float* box_center, const float* box_scale, float* center, float* scale,
                         float* confidence, int32_t* lost);

/* ---- NV12 frames (option "nv12_matrix") -----------------------------------------
 * A third frame type of the two trackers next to float32 and uint8 [B,H,W,3]: what a hardware decoder, a camera or a capture card
 * delivers.  Every NV12 entry point is DEFINED as bit-equal to its uint8 entry point on the frame hp3d_nv12_to_rgb makes.
 * Layout.  y points at frame 0's luma: H rows of `pitch` bytes, the first W of each row used.  uv points at frame 0's chroma: H/2 rows of
 *   the same pitch, U at even bytes and V at odd bytes, the first W bytes of each row used.  Frame b lies at y + b frame_stride and
 *   uv + b frame_stride (bytes).  H and W are even and at least 16 (and what every frame must satisfy); pitch >= W; B = 1 (frame_stride is
 *   then ignored) or frame_stride >= pitch (H - 1) + W.  ONLY bytes [r pitch, r pitch + W) of a row are ever read: the padding may be
 *   unmapped.
 * Pixel (r, c):  Y = y[r pitch + c],  U = uv[(r >> 1) pitch + (c & ~1)],  V = uv[(r >> 1) pitch + (c | 1)].  Chroma is REPLICATED over its
 *   2 x 2 block and not interpolated: that is the rule.
 * Conversion, exact integer arithmetic: with int32 C = Y - yoff, D = U - 128, E = V - 128 each channel is
 *   clamp((ky C + cu D + cv E + 128) >> 8, 0, 255), the shift arithmetic (floor):
 *     "nv12_matrix"          ky, yoff    R (cu, cv)   G (cu, cv)     B (cu, cv)
 *     "bt709" (default)      298, 16     0, 459       -55, -136      541, 0
 *     "bt601"                298, 16     0, 409       -100, -208     516, 0
 *     "bt709_full"           256, 0      0, 403       -48, -120      475, 0
 *     "bt601_full"           256, 0      0, 359       -88, -183      454, 0
 *   The default is bt709 because the feature is about HD video: a policy choice, not a measurement.  The rounded coefficients ARE the
 *   definition: no decoder promises these bits.  A uint8 channel becomes a network value as the uint8 path makes it: float(ch) / 255 -
 *   0.5, float32 op by op.
 * hp3d_track_step_nv12 / hp3d_track_hands_step_nv12   the planes on the host; the call uploads them (1.5 bytes a pixel; packed tight on
 *   the way).  Outputs, state and options as hp3d_track_step_u8 / hp3d_track_hands_step_u8 on the converted frames, bit for bit:
 *   "detect_scale", "track_partial_detect", "hands_compact", "track_redetect", half-precision trunks and micro-batch chunks included.
 * hp3d_track_step_nv12_dev / hp3d_track_hands_step_nv12_dev   y / uv are device pointers: the caller's surfaces are read in place,
 *   stream-ordered like hp3d_track_step_dev; every other pointer is a device pointer too.
 * What a step launches on the frame.  A TRACKED step: one crop per chunk, straight from the two planes (four conversions per output
 *   pixel; profile row "crop_and_resize_nv12", with "hands_compact" "crop_and_resize_idx_nv12"; counter "crop_nv12_launches") -- the RGB
 *   frame never exists at any size.  A DETECT step at "detect_scale" f > 1: the detection frame straight from the planes (every luma pixel
 *   of a window is converted, the three integer sums are exact; rows "downscale_nv12" / "downscale_nv12_idx"), then that crop.  A DETECT
 *   step at f = 1: the normalised float32 frame with one launch ("preprocess_nv12"; a partial detect step: the m lost frames only,
 *   "preprocess_nv12_idx"), detection and crop from it as the uint8 form does.
 * Errors, each HP3D_ERR_ARG before any launch with a message that names the argument: odd H or W, pitch < W, y or uv NULL, a
 *   frame_stride below pitch (H - 1) + W at B > 1; an unknown "nv12_matrix" is refused by hp3d_set_option.
 * Out of scope: the single-picture calls (hp3d_infer_full*, hp3d_infer_hands*) get no NV12 form; hp3d_nv12_to_rgb plus their _u8 forms
 *   serve a one-off picture.
 * The per-op forms (host pointers; the kernels run on the pitch and stride given):
 * hp3d_nv12_to_rgb            -> out [B,H,W,3] uint8 (the rule above)
 * hp3d_crop_and_resize_nv12   center [B K,2], scale [B K], K boxes per frame; idx NULL: all B K boxes -> out [B K,crop,crop,3] (m ignored);
 *                             else idx [m] slot indices in [0, B K), 0 <= m <= B K -> out [m,crop,crop,3] (crop i = box idx[i] of frame
 *                             idx[i] / K).  = hp3d_crop_and_resize_u8 / hp3d_crop_and_resize_idx on the converted frames, bit for bit
 * hp3d_downscale_nv12         f in 1 ... 8 (f = 1: the normalised frame = hp3d_preprocess_u8 at equal sizes); idx NULL: all B frames;
 *                             else idx [m] frames in [0, B), 1 <= m <= B -> out [B or m,ceil(H/f),ceil(W/f),3].  = hp3d_downscale_u8 on the
 *                             converted frames, bit for bit                                                                        */
int hp3d_track_step_nv12(hp3d_ctx* ctx, int B, int H, int W, const uint8_t* y, const uint8_t* uv, int pitch, int64_t frame_stride,
                         const float* hand_side, float* image_crop, float* scale_crop, float* center, float* keypoints_scoremap,
                         float* keypoint_coord3d, int32_t* keypoint_hw_crop, double* keypoint_hw, float* confidence, int32_t* lost,
                         int32_t* detected);
int hp3d_track_step_nv12_dev(hp3d_ctx* ctx, int B, int H, int W, const uint8_t* y, const uint8_t* uv, int pitch, int64_t frame_stride,
                             const float* hand_side, float* image_crop, float* scale_crop, float* center, float* keypoints_scoremap,
                             float* keypoint_coord3d, int32_t* keypoint_hw_crop, double* keypoint_hw, float* confidence, int32_t* lost,
                             int32_t* detected);
int hp3d_track_hands_step_nv12(hp3d_ctx* ctx, int B, int H, int W, const uint8_t* y, const uint8_t* uv, int pitch, int64_t frame_stride, int K,
                               const float* hand_side, float* image_crop, float* scale_crop, float* center, float* keypoints_scoremap,
                               float* keypoint_coord3d, int32_t* keypoint_hw_crop, double* keypoint_hw, float* confidence, int32_t* lost,
                               int32_t* detected, int32_t* valid, int32_t* area, int32_t* claimed);
int hp3d_track_hands_step_nv12_dev(hp3d_ctx* ctx, int B, int H, int W, const uint8_t* y, const uint8_t* uv, int pitch, int64_t frame_stride,
                                   int K, const float* hand_side, float* image_crop, float* scale_crop, float* center,
                                   float* keypoints_scoremap, float* keypoint_coord3d, int32_t* keypoint_hw_crop, double* keypoint_hw,
                                   float* confidence, int32_t* lost, int32_t* detected, int32_t* valid, int32_t* area, int32_t* claimed);
int hp3d_nv12_to_rgb(hp3d_ctx* ctx, const uint8_t* y, const uint8_t* uv, int B, int H, int W, int pitch, int64_t frame_stride, uint8_t* out);
int hp3d_crop_and_resize_nv12(hp3d_ctx* ctx, const uint8_t* y, const uint8_t* uv, int B, int H, int W, int pitch, int64_t frame_stride, int K,
                              const float* center, const float* scale, const int32_t* idx, int m, int crop_size, float* out);
int hp3d_downscale_nv12(hp3d_ctx* ctx, const uint8_t* y, const uint8_t* uv, int B, int H, int W, int pitch, int64_t frame_stride, int f,
                        const int32_t* idx, int m, float* out);

/* ---- packed 8-bit frames: BGR / BGRA / RGBA / ..., any pitch ---------------------
 * A fourth frame type of the two trackers: what OpenCV (BGR), GPU video post-processors, screen capture and camera SDKs (BGRA / RGBA /
 * ARGB) deliver, rows padded to a pitch, a region of interest as a view into a wider surface, on the host or -- in place -- on the
 * device.  Every packed entry point is DEFINED as bit-equal to its uint8 entry point on the frame hp3d_px_to_rgb makes: there are no
 * new numerics.
 * Layout.  px points at frame 0.  Row r of frame b starts at px + b frame_stride + r pitch (bytes); pixel c of that row starts
 *   c pixel_bytes further on.  `format`:                   pixel_bytes   byte offsets of R, G, B                                      */
#define HP3D_PX_RGB 0  /*                                    3             0, 1, 2                                                     */
#define HP3D_PX_BGR 1  /*                                    3             2, 1, 0                                                     */
#define HP3D_PX_RGBA 2 /*                                    4             0, 1, 2   (byte 3 ignored: RGBA and RGBX alike)             */
#define HP3D_PX_BGRA 3 /*                                    4             2, 1, 0   (byte 3 ignored)                                  */
#define HP3D_PX_ARGB 4 /*                                    4             1, 2, 3   (byte 0 ignored)                                  */
#define HP3D_PX_ABGR 5 /*                                    4             3, 2, 1   (byte 0 ignored)                                  */
/*   The fourth byte is never interpreted -- no premultiplication, no blending -- but it may be read.  H, W >= 16, any parity, within the
 *   frame-size limit of every frame; pitch >= W pixel_bytes; B = 1 (frame_stride is then ignored) or frame_stride >= pitch (H - 1) +
 *   W pixel_bytes.  ONLY bytes [r pitch, r pitch + W pixel_bytes) of a row are ever read: the padding may be unmapped, so a 3-byte pixel
 *   is never fetched with a 4-byte load that reaches past its row.  No alignment is required of px, pitch or frame_stride: alignment
 *   only selects a faster load (a 4-byte pixel as one 32-bit load where all three are multiples of 4; a detection window's row of
 *   2 / 4 / 8 pixels in loads of up to 16 bytes where they are multiples of the load), and both paths give the same bits.  A uint8 channel
 *   becomes a network value as the uint8 path makes it: float(ch) / 255 - 0.5, float32 op by op.
 * hp3d_track_step_px / hp3d_track_hands_step_px   the surface on the host; the call uploads it at pixel_bytes bytes a pixel (one copy
 *   where rows and frames are contiguous, packed tight on the way otherwise).  Outputs, state, counters and options as hp3d_track_step_u8 /
 *   hp3d_track_hands_step_u8 on the repacked frames, bit for bit: "detect_scale", "track_partial_detect", "track_hands_partial_detect",
 *   "hands_compact", "track_redetect", half-precision trunks and micro-batch chunks included (chunk b0 starts at px + b0 frame_stride).
 * hp3d_track_step_px_dev / hp3d_track_hands_step_px_dev   px is a device pointer: the caller's surface is read in place, stream-ordered
 *   like hp3d_track_step_dev; every other pointer is a device pointer too.  (With HP3D_PX_RGB at pitch 3 W this is the device-resident
 *   form of the uint8 entry points.)
 * What a step launches on the frame.  A TRACKED step: one crop per chunk, straight from the surface (one fetch per tap; profile row
 *   "crop_and_resize_px", with "hands_compact" "crop_and_resize_idx_px"; counter "crop_px_launches") and nothing else that reads a frame.
 *   A DETECT step at "detect_scale" f > 1: the detection frame straight from the surface (exact integer sums; rows "downscale_px" /
 *   "downscale_px_idx"), then that crop.  A DETECT step at f = 1: the normalised float32 frame with one launch ("preprocess_px"; a partial
 *   detect step: the frames that detect only, "preprocess_px_idx"), detection and crop from it as the uint8 form does.
 * Errors, each HP3D_ERR_ARG before any launch or upload with a message that names the argument: an unknown format, px NULL, pitch <
 *   W pixel_bytes, a frame_stride too short at B > 1, H or W below 16.  Counters and the profile stay untouched.
 * Out of scope: the single-picture calls (hp3d_infer_full*, hp3d_infer_hands*, hp3d_infer_2d*) get no packed form -- hp3d_px_to_rgb plus
 *   their _u8 forms serve a one-off picture; resizing on the way in (the frame size is the engine's H x W); planar RGB, 16- and 10-bit
 *   formats, alpha.
 * The per-op forms (host pointers; the surface is uploaded as it lies, so the kernels run on the pitch, stride and base misalignment
 *   -- modulo 16 -- given):
 * hp3d_px_to_rgb              -> out [B,H,W,3] uint8
 * hp3d_crop_and_resize_px     as hp3d_crop_and_resize_nv12.  = hp3d_crop_and_resize_u8 / hp3d_crop_and_resize_idx on the repacked frames
 * hp3d_downscale_px           as hp3d_downscale_nv12 (f = 1: the normalised frame).  = hp3d_downscale_u8 on the repacked frames      */
int hp3d_track_step_px(hp3d_ctx* ctx, int B, int H, int W, const uint8_t* px, int pitch, int64_t frame_stride, int format,
                       const float* hand_side, float* image_crop, float* scale_crop, float* center, float* keypoints_scoremap,
                       float* keypoint_coord3d, int32_t* keypoint_hw_crop, double* keypoint_hw, float* confidence, int32_t* lost,
                       int32_t* detected);
int hp3d_track_step_px_dev(hp3d_ctx* ctx, int B, int H, int W, const uint8_t* px, int pitch, int64_t frame_stride, int format,
                           const float* hand_side, float* image_crop, float* scale_crop, float* center, float* keypoints_scoremap,
                           float* keypoint_coord3d, int32_t* keypoint_hw_crop, double* keypoint_hw, float* confidence, int32_t* lost,
                           int32_t* detected);
int hp3d_track_hands_step_px(hp3d_ctx* ctx, int B, int H, int W, const uint8_t* px, int pitch, int64_t frame_stride, int format, int K,
                             const float* hand_side, float* image_crop, float* scale_crop, float* center, float* keypoints_scoremap,
                             float* keypoint_coord3d, int32_t* keypoint_hw_crop, double* keypoint_hw, float* confidence, int32_t* lost,
                             int32_t* detected, int32_t* valid, int32_t* area, int32_t* claimed);
int hp3d_track_hands_step_px_dev(hp3d_ctx* ctx, int B, int H, int W, const uint8_t* px, int pitch, int64_t frame_stride, int format, int K,
                                 const float* hand_side, float* image_crop, float* scale_crop, float* center, float* keypoints_scoremap,
                                 float* keypoint_coord3d, int32_t* keypoint_hw_crop, double* keypoint_hw, float* confidence, int32_t* lost,
                                 int32_t* detected, int32_t* valid, int32_t* area, int32_t* claimed);
int hp3d_px_to_rgb(hp3d_ctx* ctx, const uint8_t* px, int B, int H, int W, int pitch, int64_t frame_stride, int format, uint8_t* out);
int hp3d_crop_and_resize_px(hp3d_ctx* ctx, const uint8_t* px, int B, int H, int W, int pitch, int64_t frame_stride, int format, int K,
                            const float* center, const float* scale, const int32_t* idx, int m, int crop_size, float* out);
int hp3d_downscale_px(hp3d_ctx* ctx, const uint8_t* px, int B, int H, int W, int pitch, int64_t frame_stride, int format, int f,
                      const int32_t* idx, int m, float* out);

/* ---- a batch whose frames are separate surfaces, formats mixed --------------------
 * A fifth frame type of the two trackers, for a caller that follows one hand (or K) in each of many streams: frame b of the batch is
 * surface b -- an allocation of its own, anywhere, in any order of addresses, in its own layout (a packed format or NV12) at its own
 * pitch.  Two records may name the same surface.  No staging copy, no B calls at batch 1.
 * `surfaces` is ALWAYS an array of B records in host memory; it is read before the call returns and may be reused at once.  The
 * pointers inside the records are host pointers in the plain forms and device pointers in the _dev forms.                           */
#define HP3D_SURF_NV12 16          /* beside HP3D_PX_RGB ... HP3D_PX_ABGR (0 ... 5) */
typedef struct hp3d_surface {
    const uint8_t* data;    /* packed: byte 0 of pixel (0, 0); NV12: the luma plane                    */
    const uint8_t* chroma;  /* NV12: the interleaved chroma plane; packed formats: must be NULL        */
    int32_t pitch;          /* bytes from one row to the next (NV12: of both planes)                   */
    int32_t format;         /* HP3D_PX_* or HP3D_SURF_NV12                                             */
    int32_t height, width;  /* the picture; in this version both must equal the call's H and W         */
} hp3d_surface;
/* Definition.  Let rgb[b] = hp3d_px_to_rgb of surface b (packed) or hp3d_nv12_to_rgb of it under option "nv12_matrix" (NV12).  Every
 *   output of every entry point below equals, bit for bit, the output of the matching uint8 entry point on the stack rgb[0 .. B), under
 *   every option of the trackers ("detect_scale", "track_partial_detect", "track_hands_partial_detect", "hands_compact", "micro_batch",
 *   "track_redetect", half-precision trunks); state and counters move as the uint8 step's do.  Only the picture's bytes of a row are
 *   read, the fourth byte of a 4-byte pixel is never interpreted, and no RGB frame is made on a tracked step.  Alignment of a surface's
 *   address and pitch only selects faster loads FOR THAT SURFACE; both paths give the same bits.
 * hp3d_track_step_surf / hp3d_track_hands_step_surf   argument lists of the _px forms with (px, pitch, frame_stride, format) replaced
 *   by `surfaces`.  Host surfaces: each is uploaded tight (one copy where its rows are contiguous, packed row by row otherwise).
 * hp3d_track_step_surf_dev / hp3d_track_hands_step_surf_dev   the surfaces are read in place, stream-ordered; every other pointer is a
 *   device pointer too.  The call adds one small host-to-device copy (48 bytes a frame) and no stream synchronise.
 * Profile rows: the uint8 step's with _surf where _u8 stands ("crop_and_resize_surf", "crop_and_resize_idx_surf", "preprocess_surf[_idx]",
 *   "downscale_surf[_idx]"); counter "crop_surf_launches": one per chunk of every step that crops from the surfaces.
 * Errors, each HP3D_ERR_ARG before anything is enqueued, the tracker's state untouched, the message naming the surface index:
 *   surfaces NULL; data NULL; chroma NULL on NV12 or non-NULL on a packed format; an unknown format; pitch below the row's bytes;
 *   height / width other than H / W (mixed sizes are not supported yet); an NV12 surface with odd H or W; B < 1 or H, W < 16.
 * The per-op forms (host pointers; each surface is uploaded as it lies, at its pitch and base misalignment modulo 16):
 * hp3d_surf_to_rgb            -> out [B,H,W,3] uint8: the stack rgb[0 .. B)
 * hp3d_crop_and_resize_surf   as hp3d_crop_and_resize_px.  = hp3d_crop_and_resize_u8 / hp3d_crop_and_resize_idx on the stack
 * hp3d_downscale_surf         as hp3d_downscale_px (f in 1 ... 8; f = 1: the normalised frame).  = hp3d_downscale_u8 on the stack    */
int hp3d_track_step_surf(hp3d_ctx* ctx, int B, int H, int W, const hp3d_surface* surfaces, const float* hand_side, float* image_crop,
                         float* scale_crop, float* center, float* keypoints_scoremap, float* keypoint_coord3d, int32_t* keypoint_hw_crop,
                         double* keypoint_hw, float* confidence, int32_t* lost, int32_t* detected);
int hp3d_track_step_surf_dev(hp3d_ctx* ctx, int B, int H, int W, const hp3d_surface* surfaces, const float* hand_side, float* image_crop,
                             float* scale_crop, float* center, float* keypoints_scoremap, float* keypoint_coord3d,
                             int32_t* keypoint_hw_crop, double* keypoint_hw, float* confidence, int32_t* lost, int32_t* detected);
int hp3d_track_hands_step_surf(hp3d_ctx* ctx, int B, int H, int W, const hp3d_surface* surfaces, int K, const float* hand_side,
                               float* image_crop, float* scale_crop, float* center, float* keypoints_scoremap, float* keypoint_coord3d,
                               int32_t* keypoint_hw_crop, double* keypoint_hw, float* confidence, int32_t* lost, int32_t* detected,
                               int32_t* valid, int32_t* area, int32_t* claimed);
int hp3d_track_hands_step_surf_dev(hp3d_ctx* ctx, int B, int H, int W, const hp3d_surface* surfaces, int K, const float* hand_side,
                                   float* image_crop, float* scale_crop, float* center, float* keypoints_scoremap, float* keypoint_coord3d,
                                   int32_t* keypoint_hw_crop, double* keypoint_hw, float* confidence, int32_t* lost, int32_t* detected,
                                   int32_t* valid, int32_t* area, int32_t* claimed);
int hp3d_surf_to_rgb(hp3d_ctx* ctx, const hp3d_surface* surfaces, int B, int H, int W, uint8_t* out);
int hp3d_crop_and_resize_surf(hp3d_ctx* ctx, const hp3d_surface* surfaces, int B, int H, int W, int K, const float* center,
                              const float* scale, const int32_t* idx, int m, int crop_size, float* out);
int hp3d_downscale_surf(hp3d_ctx* ctx, const hp3d_surface* surfaces, int B, int H, int W, int f, const int32_t* idx, int m, float* out);

/* ---- per-op entry points (unit/parity tests; same kernels the pipeline runs) --------------
 * hp3d_conv2d          NetworkOps.conv/conv_relu (+ max_pool when pool=1): utils/general.py:36-65
 *                      x [B,H,W,Cin], w HWIO, SAME padding incl. the asymmetric stride-2 case.
 *                      The call describes one layer ("op/conv2d"), packs its filters and runs it through the executor's
 *                      own convolution dispatch: same kernel choice code, same launch parameters as a network layer, except
 *                      that no cost model is asked (a Winograd form runs where its option is forced to "1", F(2x2,3x3)
 *                      where the shape allows, all for Cout % 64 == 0 only) and no first-touch pass is issued.  Partial
 *                      sums of channel splits and tail pieces live in the context's scratch (grown on demand, kept until
 *                      hp3d_destroy), and with profiling on the call records its launches as rows named "op/conv2d"
 *                      (stage 1 of hp3d_get_timing).
 * hp3d_conv2d_f16      one layer of a half-precision trunk ("op/conv2d_f16"): hp3d_conv2d's construction with the executor's
 *                      dispatch in half precision, on a context of either precision, with or without finalized weights.
 *                      x and the result are float32 on the host.  The conv1_1 shape (k = 3, stride 1, 3 -> 64, no pool) is fed
 *                      the raw float32 image as in the networks; any other layer's input is rounded to half on the device
 *                      (round to nearest even) into a buffer of channel stride ceil(Cin / 64) * 64 with zero padding, its filters
 *                      are rounded to half on the host, the bias stays float32.  Sums are float32; the result is rounded to
 *                      half and widened for the caller (exact), or stays float32 with out_f32 = 1 (the score-map heads).
 *                      Kernel choice is the networks': options "f16_impl" ("h16": conv_h16.hip only where the launch fills the
 *                      chip, "h16_force": wherever the shape allows, "mfma") and "f16_k7k1"; no cost model is asked.  The call moves
 *                      "conv_h16_launches", "conv_mfma_launches", "conv_first_launches" and "conv_splitk_reduce_launches";
 *                      a shape no half-precision kernel takes (stride 2, a pooled 7x7 ...) -> HP3D_ERR_UNSUPPORTED.
 * hp3d_first_block_f16 the first block of a half-precision trunk, conv1_1 (3 -> 64) + conv1_2 (64 -> 64) + 2x2 max-pool, both
 *                      leaky-ReLU: image [B,H,W,3] float32, w1 [3,3,3,64], w2 [3,3,64,64] HWIO -> out [B,H/2,W/2,64] (halves,
 *                      widened).  One fused launch where option "f16_fuse12" ("1" | "ring" | "resident"), "f16_impl" and the
 *                      shape (even H and W) allow ("conv_h16_first_resident_launches" tells the resident form), else conv1_1
 *                      on conv_first.hip and the pooled conv1_2 through the dispatch above -- what the trunks do.
 * hp3d_maxpool2        NetworkOps.max_pool, 2x2/2 VALID                       utils/general.py:61-65
 * hp3d_avgpool8        tf.nn.avg_pool 8x8/8                                   nets/PosePriorNetwork.py:61
 * hp3d_resize_bilinear tf.image.resize_images (TF1.3 legacy bilinear)         nets/ColorHandPose3DNetwork.py:97,128,166
 * hp3d_crop_and_resize crop_image_from_xy -> tf.image.crop_and_resize         utils/general.py:163-196
 * hp3d_mask_from_scoremap single_obj_scoremap + calc_center_bb + scale        utils/general.py:233-328, CHP3D.py:82-85
 *                      Maps of up to 2^30 pixels: bit-packed maps in one workgroup's LDS where they fit (option "mask_grow",
 *                      3 * H * (ceil(W / 32) + 1) + 2 words <= 159 KB), in global scratch beyond; larger maps -> HP3D_ERR_ARG
 *                      "map too large".  With "mask_grow" = "lds" maps beyond the LDS size are refused.
 *                      -> mask [B,H,W], center [B,2], crop_size [B,1] (before *1.25), scale [B,1], seed int32 [B,2]
 * hp3d_masks_from_scoremap the mask stage of hp3d_infer_hands: scoremap [B,H,W,2], K -> mask [B,K,H,W], center [B,K,2],
 *                      crop_size [B,K], scale [B,K], seed int32 [B,K,2] ((-1, -1) for an absent slot), valid [B,K], area [B,K] int32;
 *                      same size limits and "mask_grow" forms as hp3d_mask_from_scoremap
 * hp3d_masks_from_scoremap_keep the mask stage of a multi-hand tracker's detect step (see hp3d_track_hands_step): keep int32 [B,K]
 *                      (!= 0: the slot is kept), keep_center [B,K,2], keep_scale [B,K] -> the outputs of hp3d_masks_from_scoremap with
 *                      accepted objects in the free slots and kept slots coming back as absent ones, plus claimed int32 [B,K].  With
 *                      no kept slot in an image its result is hp3d_masks_from_scoremap's bit for bit; with kept slots and an empty
 *                      detection map every free slot is absent; with no free slot the growth still runs to the end of the map or the
 *                      cap, so that claimed tells which kept slots HandSegNet still sees.
 * hp3d_fc              NetworkOps.fully_connected(_relu)                      utils/general.py:112-136
 * hp3d_argmax2d        detect_keypoints (per-channel first arg-max)           utils/general.py:331-344
 *                      x [B,H,W,C] -> int32 [B,C,2] (row, col)                                    */
int hp3d_conv2d(hp3d_ctx* ctx, const float* x, int B, int H, int W, int Cin,
                const float* w_hwio, const float* bias, int k, int stride, int Cout,
                int act, int pool, float* out);
int hp3d_conv2d_f16(hp3d_ctx* ctx, const float* x, int B, int H, int W, int Cin,
                    const float* w_hwio, const float* bias, int k, int stride, int Cout,
                    int act, int pool, int out_f32, float* out);
int hp3d_first_block_f16(hp3d_ctx* ctx, const float* image, int B, int H, int W, const float* w1, const float* b1,
                         const float* w2, const float* b2, float* out);
int hp3d_maxpool2(hp3d_ctx* ctx, const float* x, int B, int H, int W, int C, float* out);
int hp3d_avgpool8(hp3d_ctx* ctx, const float* x, int B, int H, int W, int C, float* out);
int hp3d_resize_bilinear(hp3d_ctx* ctx, const float* x, int B, int H, int W, int C,
                         int out_h, int out_w, float* out);
int hp3d_crop_and_resize(hp3d_ctx* ctx, const float* image, int B, int H, int W, int C,
                         const float* center, const float* scale, int crop_size, float* out);
int hp3d_mask_from_scoremap(hp3d_ctx* ctx, const float* scoremap, int B, int H, int W,
                            float* mask, float* center, float* crop_size, float* scale, int32_t* seed);
int hp3d_masks_from_scoremap(hp3d_ctx* ctx, const float* scoremap, int B, int H, int W, int K, float* mask, float* center,
                             float* crop_size, float* scale, int32_t* seed, int32_t* valid, int32_t* area);
int hp3d_masks_from_scoremap_keep(hp3d_ctx* ctx, const float* scoremap, int B, int H, int W, int K, const int32_t* keep,
                                  const float* keep_center, const float* keep_scale, float* mask, float* center, float* crop_size,
                                  float* scale, int32_t* seed, int32_t* valid, int32_t* area, int32_t* claimed);
int hp3d_fc(hp3d_ctx* ctx, const float* x, int B, int Cin, const float* w, const float* bias,
            int Cout, int act, float* out);
int hp3d_argmax2d(hp3d_ctx* ctx, const float* x, int B, int H, int W, int C, int32_t* out_rc);
/* detect_keypoints(tf.image.resize_images(scoremap, (out_h, out_w))[b]) for scoremap [B,h,w,C], h*w <= 4096, without
 * materialising the large map (utils/general.py:331-344 applied to nets/ColorHandPose3DNetwork.py:97): out_rc [B,C,2] */
int hp3d_detect_keypoints(hp3d_ctx* ctx, const float* scoremap, int B, int h, int w, int C, int out_h, int out_w,
                          int32_t* out_rc);

/* ---- measurement ------------------------------------------------------------------------
 * With profiling on (1: last whole-path call only, 2: accumulate over calls until switched off),
 * every launch is bracketed by hipEvents on the ctx stream.  hp3d_prof_get(i): layer name, kernel family, ms, algorithmic FLOPs and
 * algorithmic bytes (input once + weights once + output once).                */
int hp3d_set_profiling(hp3d_ctx* ctx, int on);
int hp3d_prof_count(hp3d_ctx* ctx);
int hp3d_prof_get(hp3d_ctx* ctx, int i, char* name, int name_cap, char* kernel, int kernel_cap,
                  float* ms, double* flops, double* bytes);
/* Per-stage GPU milliseconds of the profiled launches (SURVEY.md 8b `hp3d_get_timing`):
 * [0] HandSegNet, [1] mask / box / crop glue, [2] PoseNet2D (+ heat-map upsample), [3] PosePrior + ViewpointNet +
 * lifting epilogue, [4] everything.  Writes min(n, 5) values; needs hp3d_set_profiling(ctx, 1 | 2).  */
#define HP3D_TIMING_STAGES 5
int hp3d_get_timing(hp3d_ctx* ctx, float* ms_per_stage, int n);
/* Executor counters: "graph_captures" / "graph_replays" = hipGraphs instantiated / launched since hp3d_create (option
 * "graph" = "1"; a replay happens only with per-launch profiling off); "conv_h16_launches" = half-precision trunk
 * layers that ran on conv_h16.hip (option "f16_impl"); "conv_wino2_launches" = float32 layers that ran on conv_wino2.hip (option
 * "wino2"); "conv_wino4_launches" = float32 layers that ran on conv_wino4.hip (option "wino4"),
 * "conv_wino4_tail_launches" = those of them whose last round ran as channel slices (option "wino4_tail");
 * "conv_wino7_launches" = 7x7 layers that ran on conv_wino7.hip (option "wino7"), "conv_wino7_split_launches" = those of them in the channel-split form; "conv_pw2_launches" = 1x1 layer pairs that ran as one launch (option "pw2");
 * "first_touch_launches" = read passes in front of conv1_1 (option "first_touch");
 * "mask_grow_global_launches" = mask growths (one launch per call or chunk, all its images) on the global-scratch kernel (option "mask_grow");
 * "track_detect_steps" / "track_tracked_steps" = hp3d_track_step* calls that ran HandSegNet / that cropped from the previous step's keypoints;
 * "track_hands_detect_steps" / "track_hands_tracked_steps" = the same for hp3d_track_hands_step*;
 * "crop_u8_launches" = crops taken straight from a uint8 frame (tracked steps of hp3d_track_step_u8 / hp3d_track_hands_step_u8, one per chunk; hp3d_crop_and_resize_u8);
 * "detect_scale_steps" = detect steps of hp3d_track_step* / hp3d_track_hands_step* that ran at option "detect_scale" > 1; "arena_bytes" = bytes of
 * the context's frame-sized device buffers (the two activation buffers, image, staging, score map, mask, foreground, detection map);
 * "hands_compact_slots_run" / "hands_compact_slots_skipped" = slots of hp3d_infer_hands* / hp3d_track_hands_step* chunks whose back half ran / was
 * skipped under option "hands_compact" = "1", "hands_compact_waits" = stream waits for a chunk's valid flags (detect steps, hp3d_infer_hands*);
 * "track_partial_frames_run" / "track_partial_frames_skipped" = frames of hp3d_track_step* chunks that ran partially under option
 * "track_partial_detect" = "1" (0 < m < nb) on which HandSegNet ran / did not run, "frame_gather_launches" = launches of the float32 frame
 * gather (those chunks at "detect_scale" = 1 on float32 frames; hp3d_gather_frames on float32 frames at f = 1);
 * "track_hands_partial_frames_run" / "track_hands_partial_frames_skipped" = the same for hp3d_track_hands_step* chunks under option
 * "track_hands_partial_detect" = "1" (their float32 gathers count in "frame_gather_launches" too);
 * "conv_first_launches" = conv1_1-shaped layers (3x3, 3 -> 64) that ran on conv_first.hip;
 * "conv_wino_launches" = float32 layers that ran on conv_wino.hip (F(2x2,3x3), option "conv_impl" = "winograd" or the executor's choice);
 * "conv_mfma_launches" = layers that ran on the general direct kernel conv_mfma.hip (float32 and half precision);
 * "conv_splitk_reduce_launches" = channel-split reduces behind a conv_mfma / Winograd launch (whole path, hp3d_conv2d and hp3d_conv2d_f16);
 * "lift_overlap_calls" = lifting stages that ran their two towers on two streams (option "lift_overlap");
 * "lift_fused_launches" = lifting stages that ran as the one fused launch (option "lift_fused"); "comm_ranks" = ranks of the live RCCL communicator as RCCL itself
 * reports them (ncclCommCount), 0 without one -- bench.py prints it so that a multi-GPU line proves its own world size.
 * The kernel counters of the whole path ("conv_*", "first_touch_launches", "lift_fused_launches", "fc_tail_launches",
 * "mask_grow_global_launches") include the
 * launches of the second stream's half (option "streams"); "graph_*" and "lift_overlap_calls" count calls of this context. */
int hp3d_get_counter(hp3d_ctx* ctx, const char* name, long long* value);

/* ---- multi-GPU: one process and one context per GPU, RCCL over xGMI ---------
 * The path has no data-path collective.  These are the two exchanges it needs, on the context's own stream:
 * the one-off broadcast of the packed weight blob (replaces every rank un-pickling + re-packing 140 MB) and the
 * all-gather of per-shard results (keypoints: 252 B per image).  librccl is loaded on first use (dlopen), not
 * linked.  The 128-byte id is produced on one rank and handed to the others by the launcher (torch.distributed
 * store, MPI, a file ...); `hp3d_bcast_weights` on a non-root rank replaces that rank's weights (any nets mask /
 * precision the root finalized).                                                                  */
#define HP3D_COMM_ID_BYTES 128
int hp3d_comm_unique_id(void* id128);
int hp3d_comm_init(hp3d_ctx* ctx, int rank, int nranks, const void* id128);
int hp3d_bcast_weights(hp3d_ctx* ctx, int root);
int hp3d_allgather(hp3d_ctx* ctx, const float* send_host, int count, float* recv_host /* [nranks * count] */);
int hp3d_allgather_dev(hp3d_ctx* ctx, const float* send_dev, int count, float* recv_host /* [nranks * count] */);
int hp3d_comm_destroy(hp3d_ctx* ctx);

/* ---- memory for callers that keep their batches in HBM (the `_dev` entry points; bench.py, hand3d_amd/dist.py) ---
 * Replaces what the reference left to TensorFlow's feed_dict / allocator (run.py:61-64): device buffers, pinned host
 * buffers, blocking copies ordered on the context's stream (kind 0 = host->device, 1 = device->host, 2 = device->
 * device), and an upload on a SECOND stream so that the host->device copy of batch n+1 runs under the kernels of
 * batch n (hp3d_wait_upload makes the compute stream wait for the last hp3d_upload_async).  No PyTorch needed.     */
int hp3d_dev_alloc(hp3d_ctx* ctx, size_t bytes, void** out);
int hp3d_dev_free(hp3d_ctx* ctx, void* p);
int hp3d_host_alloc(hp3d_ctx* ctx, size_t bytes, void** out);      /* page-locked */
int hp3d_host_free(hp3d_ctx* ctx, void* p);
int hp3d_memcpy(hp3d_ctx* ctx, void* dst, const void* src, size_t bytes, int kind);
int hp3d_upload_async(hp3d_ctx* ctx, void* dst_dev, const void* src_pinned_host, size_t bytes);
int hp3d_wait_upload(hp3d_ctx* ctx);

/* ---- host utility ----------------------------------------------------------------------------
 * CRC-32C (Castagnoli) of a host buffer: the checksum TensorFlow checkpoints carry (hand3d_amd/utils/tf_checkpoint.py
 * verifies 140 MB of tensors with it; the pure-Python loop manages ~5 MB/s).  No device involved.          */
uint32_t hp3d_crc32c(const void* data, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* HP3D_H */
