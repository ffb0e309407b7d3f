// engine.hip -- context, weight packing, stream-ordered executor and the C-ABI of libhp3d.so.
// Host code only (the kernels live in conv_mfma.hip / glue.hip).  See include/hp3d.h for the
// reference interfaces each entry point replaces.
// One convolution path: reserve_conv lays a layer's filter sections out, pack_layer fills them, run_conv picks the kernel and launches
// it.  The networks' layers live in the context's blob (Tables); hp3d_conv2d describes its one layer, packs it into a scratch blob and
// calls the same run_conv -- of its own it only chooses which sections that layer has.
#include "hp3d_common.h"
#include "lift_fused.h"
#include "../../include/hp3d.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <thread>
#include <chrono>
#include <atomic>
#include <functional>
#include <string>
#include <vector>
#ifndef HP3D_EMU
#include <dlfcn.h>
#include <rccl/rccl.h>      // types and prototypes only: the library is dlopen'ed on first use (573 MB), never linked
#endif

namespace {

std::string g_last_error;

#define HP3D_FAIL(ctx, code, ...)                              \
    do {                                                       \
        char _b[512];                                          \
        snprintf(_b, sizeof(_b), __VA_ARGS__);                 \
        set_error((ctx), _b);                                  \
        return (code);                                         \
    } while (0)
#define HIPCHK(ctx, expr)                                                                          \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) HP3D_FAIL(ctx, HP3D_ERR_HIP, "%s -> %s", #expr, hipGetErrorString(_e)); \
    } while (0)
#define CHK(expr)                     \
    do {                              \
        int _r = (expr);              \
        if (_r != 0) return _r;       \
    } while (0)

enum { NET_SEG = 1, NET_POSE = 2, NET_PRIOR = 4, NET_VP = 8, NET_BOTTLENECK = 16 };

// ---- layer tables (mirror hand3d_amd/arch.py; nets/ColorHandPose3DNetwork.py:144-161,183-214,255-267,291-307)
struct ConvL {
    std::string name;      // tf scope/layer, e.g. "HandSegNet/conv1_2"
    int k, cin, cout, stride, relu;
    int mode;              // 0 plain, 1 im2col first layer (Cin=3), 2 concat-permuted (conv6_1/conv7_1)
    // packed geometry
    int ek, cin_pad, cout_pad;
    size_t w_off, b_off;   // offsets into the blob (floats)
    size_t ww_off = 0;     // Winograd-transformed filters U[16][cin_pad][cout_pad] (3x3/s1, cout%64==0), 0 = none
    size_t ww2_off = 0;    // the same filters in conv_wino2.hip's fragment order (two workgroups per CU), 0 = none
    size_t ww4_off = 0;    // F(4x4,3x3) filters U[36][...] in conv_wino4.hip's fragment order (trunk nets), 0 = none
    size_t ww4s_off = 0;   // the F(4x4,3x3) filters split into three bfloat16 pieces in conv_wino4s.hip's fragment order (3x3 trunk layers with Cin >= 128), 0 = none
    size_t ww7_off = 0;    // 7x7 layers: F(4x4,4x4) filters of the four 4x4-tap blocks in conv_wino7.hip's order [chunk][169][Cout/16][q][n][e], 0 = none
    size_t raw_off = 0;    // lifting nets only: [Cout/64][cin4][tap][64] for lift_fused.hip (one contiguous weight stream per wave), 0 = none
    size_t hwio_off = 0;   // lifting nets, the last stride-2 layer of a tower (8x8 -> 4x4 map): the plain HWIO filter = the matrix of conv_s2_gemm_launch, 0 = none
    int cin4 = 0;
    int cin_pad16 = 0;     // f16 mode: input channels padded to 64 halves (one 128-B chunk)
    size_t w16_off = 0;    // offset into the f16 blob (halves); trunk nets only
    int net;
};
struct FcL {
    std::string name;
    int cin, cout, relu;
    size_t w_off, b_off;
    int net;
};

int pad32(int c) { return (c + 31) / 32 * 32; }

// The optional sections of a layer's packed filters.  Which of them a layer carries is its owner's choice (Tables::add_conv for the
// networks, hp3d_conv2d for its one layer); how large and how aligned each one is, is reserve_conv's alone.
enum { SEC_WINO = 1, SEC_WINO2 = 2, SEC_WINO4 = 4, SEC_WINO7 = 8, SEC_WINO4S = 16, SEC_RAW = 32, SEC_HWIO = 64, SEC_F16 = 128 };

// Lays the direct filters, the bias and the sections `secs` of layer l (k, cin, cout, mode, ek, cin_pad, cout_pad set) out behind
// `floats`, the half-precision filters behind `halves`.  An absent section keeps offset 0: behind the direct filters no section starts there.
void reserve_conv(ConvL& l, int secs, size_t& floats, size_t& halves) {
    auto take = [&](size_t n, bool align16 = false) {
        if (align16) floats = (floats + 3) / 4 * 4;
        const size_t off = floats;
        floats += n;
        return off;
    };
    l.w_off = take((size_t)l.ek * l.ek * l.cin_pad * l.cout_pad);
    l.b_off = take(l.cout_pad);
    // Winograd F(2x2,3x3) copies (16 planes; a 7x7 filter as nine 3x3 blocks along the channel axis)
    if (secs & SEC_WINO) l.ww_off = take(wino_packed_floats(l.k, l.cin_pad, l.cout_pad));
    if (secs & SEC_WINO2) l.ww2_off = take(wino_packed_floats(l.k, l.cin_pad, l.cout_pad));
    if (secs & SEC_WINO4) l.ww4_off = take(wino4_packed_floats(l.k, l.cin_pad, l.cout_pad));
    if (secs & SEC_WINO7) l.ww7_off = take(wino7_packed_floats(l.cin_pad, l.cout_pad));
    if (secs & SEC_WINO4S) l.ww4s_off = take((wino4s_packed_bytes(l.cin_pad, l.cout_pad) + 15) / 16 * 4, true);
    if (secs & SEC_RAW) {
        l.cin4 = (l.cin + 15) / 16 * 16;          // four waves x whole channel quads
        l.raw_off = take((size_t)9 * l.cin4 * ((l.cout + 63) / 64 * 64));
    }
    if (secs & SEC_HWIO) l.hwio_off = take((size_t)9 * l.cin * l.cout, true);
    if (secs & SEC_F16) {
        l.cin_pad16 = (l.mode == 1) ? 64 : (l.mode == 2) ? 192 : (l.cin + 63) / 64 * 64;
        l.w16_off = halves;
        halves += (size_t)l.ek * l.ek * l.cin_pad16 * l.cout_pad;
    }
}

struct Tables {
    std::vector<ConvL> conv;
    std::vector<FcL> fc;
    std::map<std::string, int> conv_idx, fc_idx;
    size_t blob_floats = 0, blob16_halves = 0;

    void add_conv(const char* scope, const char* name, int k, int cin, int cout, int stride, int relu, int net) {
        ConvL l;
        l.name = std::string(scope) + "/" + name;
        l.k = k; l.cin = cin; l.cout = cout; l.stride = stride; l.relu = relu; l.net = net;
        l.mode = (cin == 3) ? 1 : (cin == 149) ? 2 : 0;
        l.ek = (l.mode == 1) ? 1 : k;
        l.cin_pad = (l.mode == 1) ? 32 : (l.mode == 2) ? 160 : pad32(cin);
        l.cout_pad = pad32(cout);
        const bool trunk = net == NET_SEG || net == NET_POSE;
        int secs = 0;
        if (stride == 1 && cout % 64 == 0 && ((k == 3 && l.mode == 0) || (k == 7 && (l.mode == 0 || l.mode == 2)))) {
            secs |= SEC_WINO | SEC_WINO2;
            if (trunk) secs |= SEC_WINO4 | (k == 7 ? SEC_WINO7 : 0) | (k == 3 && l.mode == 0 && l.cin_pad >= 128 && l.cin_pad % 16 == 0 ? SEC_WINO4S : 0);
        }
        if (net == NET_PRIOR || net == NET_VP) secs |= SEC_RAW;         // lift_fused.hip's weight streams
        if (net == NET_VP && stride == 2 && k == 3 && cin >= 256) secs |= SEC_HWIO;         // (ViewpointNet/conv_vp_2_2: 47 -> 39 us; PosePrior's 128-channel twin measured slower this way)
        if (trunk) secs |= SEC_F16;                 // half-precision copy for hp3d_finalize_weights(dtype=1)
        reserve_conv(l, secs, blob_floats, blob16_halves);
        conv_idx[l.name] = (int)conv.size();
        conv.push_back(l);
    }
    void add_fc(const char* scope, const char* name, int cin, int cout, int relu, int net) {
        FcL l;
        l.name = std::string(scope) + "/" + name;
        l.cin = cin; l.cout = cout; l.relu = relu; l.net = net;
        l.w_off = blob_floats;
        blob_floats += ((size_t)cin * cout + 3) / 4 * 4;
        l.b_off = blob_floats;
        blob_floats += (cout + 3) / 4 * 4;
        fc_idx[l.name] = (int)fc.size();
        fc.push_back(l);
    }
    Tables() {
        char nm[32];
        {   // HandSegNet
            const int nl[4] = {2, 2, 4, 4}, ch[4] = {64, 128, 256, 512};
            int cin = 3;
            for (int b = 0; b < 4; ++b)
                for (int i = 0; i < nl[b]; ++i) {
                    snprintf(nm, sizeof nm, "conv%d_%d", b + 1, i + 1);
                    add_conv("HandSegNet", nm, 3, cin, ch[b], 1, 1, NET_SEG);
                    cin = ch[b];
                }
            add_conv("HandSegNet", "conv5_1", 3, 512, 512, 1, 1, NET_SEG);
            add_conv("HandSegNet", "conv5_2", 3, 512, 128, 1, 1, NET_SEG);
            add_conv("HandSegNet", "conv6_1", 1, 128, 512, 1, 1, NET_SEG);
            add_conv("HandSegNet", "conv6_2", 1, 512, 2, 1, 0, NET_SEG);
        }
        {   // PoseNet2D
            const int nl[4] = {2, 2, 4, 2}, ch[4] = {64, 128, 256, 512};
            int cin = 3;
            for (int b = 0; b < 4; ++b)
                for (int i = 0; i < nl[b]; ++i) {
                    snprintf(nm, sizeof nm, "conv%d_%d", b + 1, i + 1);
                    add_conv("PoseNet2D", nm, 3, cin, ch[b], 1, 1, NET_POSE);
                    cin = ch[b];
                }
            add_conv("PoseNet2D", "conv4_3", 3, 512, 256, 1, 1, NET_POSE);
            add_conv("PoseNet2D", "conv4_4", 3, 256, 256, 1, 1, NET_POSE);
            add_conv("PoseNet2D", "conv4_5", 3, 256, 256, 1, 1, NET_POSE);
            add_conv("PoseNet2D", "conv4_6", 3, 256, 256, 1, 1, NET_POSE);
            add_conv("PoseNet2D", "conv4_7", 3, 256, 128, 1, 1, NET_POSE);
            add_conv("PoseNet2D", "conv5_1", 1, 128, 512, 1, 1, NET_POSE);
            add_conv("PoseNet2D", "conv5_2", 1, 512, 21, 1, 0, NET_POSE);
            for (int p = 6; p <= 7; ++p) {
                int c = 149;
                for (int r = 1; r <= 5; ++r) {
                    snprintf(nm, sizeof nm, "conv%d_%d", p, r);
                    add_conv("PoseNet2D", nm, 7, c, 128, 1, 1, NET_POSE);
                    c = 128;
                }
                snprintf(nm, sizeof nm, "conv%d_6", p);
                add_conv("PoseNet2D", nm, 1, 128, 128, 1, 1, NET_POSE);
                snprintf(nm, sizeof nm, "conv%d_7", p);
                add_conv("PoseNet2D", nm, 1, 128, 21, 1, 0, NET_POSE);
            }
        }
        {   // PosePrior
            const int ch[3] = {32, 64, 128};
            int cin = 21;
            for (int i = 0; i < 3; ++i) {
                snprintf(nm, sizeof nm, "conv_pose_%d_1", i);
                add_conv("PosePrior", nm, 3, cin, ch[i], 1, 1, NET_PRIOR);
                snprintf(nm, sizeof nm, "conv_pose_%d_2", i);
                add_conv("PosePrior", nm, 3, ch[i], ch[i], 2, 1, NET_PRIOR);
                cin = ch[i];
            }
            add_fc("PosePrior", "fc_rel0", 2050, 512, 1, NET_PRIOR);
            add_fc("PosePrior", "fc_rel1", 512, 512, 1, NET_PRIOR);
            add_fc("PosePrior", "fc_xyz", 512, 63, 0, NET_PRIOR);
            add_fc("PosePrior", "fc_bottleneck", 512, 30, 0, NET_BOTTLENECK);
            add_fc("PosePrior", "fc_xyz#bn", 30, 63, 0, NET_BOTTLENECK);   // fc_xyz of the bottleneck variant
        }
        {   // ViewpointNet
            const int ch[3] = {64, 128, 256};
            int cin = 21;
            for (int i = 0; i < 3; ++i) {
                snprintf(nm, sizeof nm, "conv_vp_%d_1", i);
                add_conv("ViewpointNet", nm, 3, cin, ch[i], 1, 1, NET_VP);
                snprintf(nm, sizeof nm, "conv_vp_%d_2", i);
                add_conv("ViewpointNet", nm, 3, ch[i], ch[i], 2, 1, NET_VP);
                cin = ch[i];
            }
            add_fc("ViewpointNet", "fc_vp0", 4098, 256, 1, NET_VP);
            add_fc("ViewpointNet", "fc_vp1", 256, 128, 1, NET_VP);
            // fc_vp_ux / uy / uz ([128,1] each) are packed as one [128,3] matrix
            add_fc("ViewpointNet", "fc_vp_u", 128, 3, 0, NET_VP);
        }
    }
};

struct HostVar {
    std::vector<float> data;
    std::vector<int64_t> shape;
};

struct ProfRec {
    std::string name, kernel;
    double flops, bytes;
    hipEvent_t e0, e1;
};

// Everything hp3d_set_option writes.  The second stream's context copies the whole record (kid_sync_state), so an option added
// here reaches both halves of a two-stream call.
struct Options {
    int empty_fltmax = 0;
    int conv_naive = 0;
    int use_wino = 1;          // 3x3/s1 layers with Cout%64==0 run as Winograd F(2x2,3x3) (conv_impl=direct disables)
    int first_touch_beside = 1;     // option "first_touch_beside": the read pass on the child context's stream beside conv1_1 (1) | in front of it (0)
    int first_touch = -1;      // option "first_touch": stream conv1_1's input image through the memory-side cache right before the launch: -1 auto
                               // (a cold image of 8 ... 128 MB), 0 never, 1 always
    int first_balanced = 1;    // option "first_walk": conv_first.hip's workgroups walk balanced runs of tiles ("balanced") | whole tile rows ("rows": rounds 2-4)
    int use_first = 1;         // conv1_1 on its own kernel (conv_first.hip); conv_impl=direct keeps it on the general one
    int nstreams = -1;         // whole-path calls: halves of the batch on two HIP streams (option "streams"; -1 auto)
    int use_h16 = 1;           // half-precision 3x3 trunk layers on conv_h16.hip (option "f16_impl" = "h16" | "mfma")
    int h16_k7k1 = 1;          // ... and the 7x7 / 1x1 layers with >= 64 couts on its single-buffer forms (option "f16_k7k1" = 0 | 1)
    int wino_splitk = 1;       // Winograd layers that under-fill the chip split their channel steps (option "wino_splitk")
    int lift_overlap = 1;      // option "lift_overlap": the two towers of the unfused lifting stage on two streams (ViewpointNet on the child context's)
    int use_lift_fused = -1;   // the lifting stage as one launch (lift_fused.hip): -1 auto (B <= 4), 0 never, 1 always (option "lift_fused")
    int use_wino2 = -1;        // conv_wino2.hip (two workgroups per CU): -1 auto (short reductions, under-filled launches), 0 never, 1 wherever eligible (option "wino2")
    int use_graph = 0;
    int fuse12 = 1;            // half-precision trunks: conv1_1 computed inside conv1_2's patch stage (option "f16_fuse12": 0 | 1 = form by size |
                               // 2 = "ring": two workgroups per CU, filter ring | 3 = "resident": one per CU, conv1_2's filters in registers)
    int use_wino4 = -2;        // conv_wino4.hip (Winograd F(4x4,3x3)), option "wino4": -2 auto (both trunks by cost model), -1 "pose" (PoseNet2D only, by cost
                               // model), 0 never, 1 wherever eligible (tests)
    int use_wino4s = 0;        // conv_wino4s.hip (F(4x4,3x3) on the bf16 matrix pipe, split operands), option "wino4_split": 0 never, -1 "auto" (the filled
                               // 3x3 launches with Cin >= 128 that conv_wino4.hip would take), 1 wherever eligible (tests)
    int kp_up_side = 1;        // the heat-map up-sampling behind ViewpointNet on the child stream (1) or behind PosePrior on this one (0): option "kp_up_side"
    int fc_tail = 1;           // the tail of a lifting tower (reduce of the first FC layer + the two small FC layers) as one launch (option "fc_tail")
    int tiny_gemm = 1;         // the towers' last stride-2 layer (8x8 -> 4x4) as split-K GEMM over its output pixels (option "tiny_gemm")
    int w4_tail = 1;           // conv_wino4.hip: cut an under-filled last round of items into channel slices (option "wino4_tail")
    int use_pw2 = 1;           // conv_pw2.hip: the 1x1 head pairs (conv6_1 + conv6_2, conv5_1 + conv5_2, conv6_6 + conv6_7, conv7_6 + conv7_7) as one launch each
                               // (option "pw2": 0 never, 1 when the launch has a workgroup per CU, 2 = "force": whenever the shapes allow, tests)
    int use_wino7 = -1;        // conv_wino7.hip (the 7x7 layers as Winograd F(4x4,4x4)), option "wino7": -1 auto (launches that fill the chip), 0 never, 1 wherever eligible
    int wino7_ksplit = 0;      // option "wino7_ksplit": 0 = auto (conv_wino7_eligible's choice for under-filled launches), N = that many channel splits (tests, tuning)
    int mask_grow = 0;         // option "mask_grow": 0 "auto" (mask_grow_kernel where its LDS maps fit, the global-scratch kernel beyond), 1 "lds"
                               // (the LDS kernel only: larger frames are refused), 2 "global" (the global-scratch kernel at every size)
    int micro_batch = -1;      // whole-path calls run in chunks of at most this many images (0: never split; -1 auto:
                               // 32 in float32 mode, no split with half-precision trunks -- measured optima)
    float track_margin = 1.25f;     // option "track_margin": factor on the tracked box's size (the detection path's own 1.25, ColorHandPose3DNetwork.py:84)
    float track_min_score = 0.f;    // option "track_min_score": a tracked image is lost when its confidence is below this ...
    int track_use_min_score = 0;    // ... "off" (default): never
    int track_redetect = 0;         // option "track_redetect": every N-th tracking step is a detect step that re-boxes every image (0: never)
    int hands_min_area = 0;         // option "hands_min_area": hp3d_infer_hands* / hp3d_masks_from_scoremap drop objects of fewer pixels (0: off)
    int detect_scale = 1;           // option "detect_scale": the detect steps of hp3d_track_step* / hp3d_track_hands_step* find the hand on the frame's
                                    // f x f area mean and crop from the frame itself (1: detect on the frame)
    int hands_compact = 0;          // option "hands_compact": hp3d_infer_hands* / hp3d_track_hands_step* run the back half on the slots that hold a
                                    // hand only; 0: every slot runs, absent ones on their fall-back crop
    int track_partial_detect = 0;   // option "track_partial_detect": a detect step of hp3d_track_step* that only `lost` flags caused runs HandSegNet,
                                    // the soft-max and the mask growth on the lost frames only; 0: on the whole batch
    int track_hands_partial_detect = 0;   // option "track_hands_partial_detect": the same for hp3d_track_hands_step* -- on the frames that have a valid
                                    // slot lost or no valid slot; 0: on the whole batch
    int nv12_matrix = 0;            // option "nv12_matrix": the colour matrix of NV12 frames: 0 "bt709" (default), 1 "bt601",
                                    // 2 "bt709_full", 3 "bt601_full" (nv12_matrix_index)
};

// Launch counters (hp3d_get_counter: which kernels really ran).
struct Counters {
    long conv_first_launches = 0;
    long first_touch_launches = 0;
    long lift_overlap_calls = 0;
    long lift_fused_launches = 0;
    long graph_captures = 0, graph_replays = 0;     // did the hipGraph path really run?
    long conv_h16_first_resident_launches = 0;
    long conv_h16_launches = 0;                     // layers that went to conv_h16.hip
    long conv_wino4s_launches = 0;
    long conv_wino4s_tail_launches = 0;
    long fc_tail_launches = 0, conv_s2_gemm_launches = 0;
    long conv_pw2_launches = 0;
    long conv_wino7_launches = 0;
    long conv_wino7_split_launches = 0;
    long conv_wino4_tail_launches = 0;
    long conv_wino4_launches = 0;                   // layers that went to conv_wino4.hip
    long conv_wino2_launches = 0;                   // layers that went to conv_wino2.hip
    long conv_wino_launches = 0;                    // layers that went to conv_wino.hip
    long conv_mfma_launches = 0;                    // layers that went to the general direct kernel (conv_mfma.hip, f32 and f16)
    long conv_splitk_reduce_launches = 0;           // channel-split reduces (conv_splitk_reduce*_launch)
    long mask_grow_global_launches = 0;             // mask growths on the global-scratch kernel
    long mask_grow_multi_launches = 0;              // mask growths of the multi-hand kernels (either form)
    long track_detect_steps = 0, track_tracked_steps = 0;      // hp3d_track_step*: steps that ran HandSegNet / that did not
    long crop_u8_launches = 0;                      // crops taken straight from a uint8 frame (crop_and_resize_u8_kernel)
    long track_hands_detect_steps = 0, track_hands_tracked_steps = 0;      // hp3d_track_hands_step*: as track_*_steps
    long detect_scale_steps = 0;                    // detect steps of either tracker that ran at detect_scale > 1
    long hands_compact_slots_run = 0, hands_compact_slots_skipped = 0;     // option "hands_compact": slots whose back half ran / was skipped
    long hands_compact_waits = 0;                   // ... and the stream waits for a chunk's valid flags (detect steps, hp3d_infer_hands*)
    long track_partial_frames_run = 0, track_partial_frames_skipped = 0;   // option "track_partial_detect": frames of partial chunks HandSegNet ran on / did not
    long frame_gather_launches = 0;                 // ... and the launches of frame_gather_kernel (the step and hp3d_gather_frames)
    long track_hands_partial_frames_run = 0, track_hands_partial_frames_skipped = 0;   // option "track_hands_partial_detect": the same
    long crop_nv12_launches = 0;                    // crops taken straight from an NV12 frame (either crop_and_resize*_nv12_kernel)
    long crop_px_launches = 0;                      // crops taken straight from a packed 8-bit frame (either crop_and_resize*_px_kernel)
    long crop_surf_launches = 0;                    // crops taken straight from a batch of surfaces (either crop_and_resize*_surf_kernel)
};

// A page-locked int buffer that small copies fill or drain behind the stream (the trackers' flags, the compaction's maps), the event
// behind the last of them and whether it has been waited for.  The host touches h only after wait().
struct HostFlags {
    int* h = nullptr;
    hipEvent_t ev = nullptr;
    bool pending = false;
    int resize(hp3d_ctx* ctx, size_t n, const char* what);          // n ints, contents undefined; the caller has waited
    int wait(hp3d_ctx* ctx);
    int record(hp3d_ctx* ctx);                    // a copy that reads or writes h has just been enqueued
    int copy_behind(hp3d_ctx* ctx, const int* d_src, size_t n);      // h <- n ints of the device, behind the stream
    void free();
};

// Option "hands_compact" (DESIGN.md 4.15).  map: two page-locked buffers used in turn, idx [cap] | pos [cap] of one chunk; a buffer is
// rewritten only after the event behind its last upload.  d_map: the same on the device (stream order protects it).
struct CompactBufs {
    int cap = 0;                        // slots the buffers hold
    HostFlags map[2];
    int turn = 0;
    HostFlags valid;                    // a chunk's valid flags (detect steps, hp3d_infer_hands*)
    int* d_map = nullptr;
    float *d_hs = nullptr, *d_center = nullptr, *d_scale = nullptr;      // hand_side / centre / scale of the slots that run, dense
};

// A batch of separate surfaces.  d_rec: the device table, one SurfRec per frame (stream order protects it).  stage: two
// page-locked buffers of records used in turn; a buffer is rewritten only after the event behind its last upload, so a _dev step never
// waits for the step in front of it.
struct SurfTable {
    int cap = 0;                        // records the buffers hold
    SurfRec* d_rec = nullptr;
    HostFlags stage[2];
    int turn = 0;
};

// What a context knows about the hands it follows (hp3d_track_*): the boxes for the next step, on the device, and the host's copy of the
// `lost` flags that decides whether the next step detects.  Two box buffers: a step crops from box[cur] and writes the next boxes to
// box[cur ^ 1], so the boxes a step used are still there when its outputs are copied out.
struct TrackState {
    int cap = 0;                        // images the buffers hold
    float* center[2] = {nullptr, nullptr};
    float* scale[2] = {nullptr, nullptr};
    float* conf = nullptr;
    int *lost = nullptr, *detected = nullptr;
    int *pidx = nullptr, *ppos = nullptr;      // option "track_partial_detect": per chunk at its offset, the lost frames' indices in the chunk | a frame's dense index
    HostFlags h_lost;                   // the last step's flags, copied behind the step
    int cur = 0;
    bool valid = false;                 // box[cur] holds boxes for (B, H, W)
    int B = 0, H = 0, W = 0;
    int f = 1;                          // ... found at this detect_scale (a change counts as a change of shape)
    int since = 0;                      // tracked steps since the last detect step
};

// The multi-hand tracker's state (hp3d_track_hands_*): the same per slot (b, j) at index b * K + j, separate from
// TrackState.  flags = valid [n] | lost [n] (n = B * K slots of the current shape), so that one 8 n-byte copy carries both to the host.
struct TrackHandsState {
    int cap = 0;                        // slots the buffers hold
    float* center[2] = {nullptr, nullptr};
    float* scale[2] = {nullptr, nullptr};
    float* conf = nullptr;
    int *flags = nullptr, *detected = nullptr, *area = nullptr, *claimed = nullptr;
    int* keep = nullptr;                // valid and not lost after the last step: what a detect step behind it keeps
    // option "track_hands_partial_detect" (grown by ensure_track_hands_partial): per chunk at its frame offset, the detecting frames'
    // indices in the chunk | a frame's dense index; keep / centre / scale of a chunk's detecting frames, dense, and the growth's claimed
    int pcap = 0;
    int *pidx = nullptr, *ppos = nullptr, *keep_d = nullptr, *claimed_d = nullptr;
    float *center_d = nullptr, *scale_d = nullptr;
    HostFlags h_flags;                  // the last step's valid | lost, copied behind the step
    int cur = 0;
    bool ok = false;                    // box[cur] and the flags hold a state for (B, K, H, W)
    int B = 0, K = 0, H = 0, W = 0;
    int f = 1;                          // the detect_scale of that state (a change counts as a change of shape)
    int since = 0;                      // tracked steps since the last detect step
    int* valid() const { return flags; }
    int* lost() const { return flags + (size_t)B * K; }
};

}  // namespace

struct hp3d_ctx : Options, Counters {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    Tables T;
    std::map<std::string, HostVar> vars;
    float* blob = nullptr;     // device, T.blob_floats
    hp3d_f16* blob16 = nullptr; // device, T.blob16_halves (dtype 1 only)
    int prec = 0;              // 0: f32 everywhere; 1: HandSegNet / PoseNet2D trunks in f16 (f32 accumulate)
    hp3d_f16* d_concat16 = nullptr;
    size_t concat16_px = 0;
    int nets = 0;              // finalized nets mask
    // debug copies of the unpacked HWIO weights for conv_impl=naive
    std::map<std::string, float*> naive_w;

    // arena
    size_t act_floats = 0;     // capacity of bufA/bufB
    float *bufA = nullptr, *bufB = nullptr, *col = nullptr;
    size_t col_floats = 0;
    int capB = 0;
    int sideB = 0;             // batch the FC buffers hold when this context is only the side tower of an overlapped lifting stage (ensure_side_tower)
    float *d_image = nullptr, *d_hs = nullptr, *d_large = nullptr, *d_crop = nullptr, *d_center = nullptr,
          *d_scale = nullptr, *d_cropsize = nullptr, *d_kpmap = nullptr, *d_coord = nullptr, *d_mask = nullptr,
          *d_segsmall = nullptr, *d_concat = nullptr, *d_sm[3] = {nullptr, nullptr, nullptr}, *d_can = nullptr,
          *d_rot = nullptr, *d_u = nullptr, *d_fc1 = nullptr, *d_fc2 = nullptr, *d_fg = nullptr,
          *d_pooled = nullptr, *d_fcpart = nullptr;
    float* d_stage = nullptr;            // detect_scale > 1: a host float32 frame at full size (d_image holds the detection frame)
    size_t stage_floats = 0;
    float *d_keepc = nullptr, *d_keeps = nullptr;      // detect_scale > 1: the kept slots' boxes in detection-frame coordinates
    hipStream_t copy_stream = nullptr;   // hp3d_upload_async: H2D of the next batch under the current batch's kernels
    hipEvent_t upload_done = nullptr;
    double* d_kpimg = nullptr;   // [B,21,2] float64 (trafo_coords of the detected keypoints)
    int* d_kpcrop = nullptr;     // [B,21,2] int32 (detect_keypoints: row, col in the crop)
    void* comm = nullptr;        // ncclComm_t (hp3d_comm_init)
    float* d_gather = nullptr;   // reusable send + receive staging of hp3d_allgather[_dev] (no allocation per step)
    size_t gather_floats = 0;
    int comm_rank = 0, comm_size = 1;
    int* d_seed = nullptr;
    int *d_valid = nullptr, *d_area = nullptr;      // hp3d_infer_hands*: per slot
    size_t mask_floats = 0;                         // capacity of d_mask
    unsigned long long* d_keys = nullptr;
    unsigned char* d_det = nullptr;
    unsigned char* d_u8 = nullptr;
    size_t u8_bytes = 0;
    std::vector<unsigned char> h_nv12;               // host NV12 planes with a pitch above W, packed tight for their upload
    std::vector<unsigned char> h_px;                 // host packed 8-bit frames with padded rows or frames, likewise
    size_t image_floats = 0, large_floats = 0, det_bytes = 0, pose_px = 0;

    // profiling
    int profiling = 0;
#ifndef HP3D_EMU
    struct GraphEntry { hipGraphExec_t exec = nullptr; long epoch = -1; int calls = 0; };
    std::map<std::string, GraphEntry> graphs;    // hp3d_set_option("graph", "1"): replayed whole-call launch sequences
#endif
    bool trunk_input_hot = false;   // set by run_trunk: the trunk's input was written by the kernel in front of it (crop, uint8 front end)
    hp3d_ctx* kid = nullptr;   // the second stream's context: own stream + arena, SHARES this context's weight blob
    bool shared_weights = false;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    unsigned* d_liftbar = nullptr;
    unsigned* h_lifterr = nullptr;     // mapped host word: lift_fused.hip's grid barrier timed out (results of that launch are invalid)
    bool two_streams_live = false;   // set while a whole-path call runs its two halves on two streams (kernel choice: wino2_auto)
    long graph_epoch = 0;      // bumped by anything a captured sequence depends on (allocations, weights, options)
    unsigned* d_mgscratch = nullptr;                // the global-scratch kernel's bitmaps, B x mask_grow_global_words(H, W) words
    size_t mg_words = 0;
    TrackState track;
    TrackHandsState track_hands;
    CompactBufs compact;
    SurfTable surf;
    std::vector<ProfRec> prof;
    std::vector<hipEvent_t> event_pool;
    size_t event_next = 0;
};

namespace {

void set_error(hp3d_ctx* ctx, const char* msg) {
    g_last_error = msg;
    if (ctx) ctx->err = msg;
}

template <typename T>
int dev_realloc(hp3d_ctx* ctx, T** p, size_t count) {
    ++ctx->graph_epoch;            // captured launch sequences hold the old address
    if (*p) hipFree(*p);
    *p = nullptr;
    HIPCHK(ctx, hipMalloc((void**)p, count * sizeof(T)));
    return 0;
}

hipEvent_t get_event(hp3d_ctx* ctx) {
    if (ctx->event_next == ctx->event_pool.size()) {
        hipEvent_t e;
        hipEventCreate(&e);
        ctx->event_pool.push_back(e);
    }
    return ctx->event_pool[ctx->event_next++];
}

struct ProfScope {          // kernel == nullptr: no profile row
    hp3d_ctx* ctx;
    int idx = -1;
    ProfScope(hp3d_ctx* c, const std::string& name, const char* kernel, double flops, double bytes) : ctx(c) {
        if (!c->profiling || !kernel) return;
        ProfRec r{name, kernel, flops, bytes, get_event(c), get_event(c)};
        hipEventRecord(r.e0, c->stream);
        idx = (int)c->prof.size();
        c->prof.push_back(r);
    }
    ~ProfScope() {
        if (idx >= 0) hipEventRecord(ctx->prof[idx].e1, ctx->stream);
    }
};

void prof_reset(hp3d_ctx* ctx) {
    ctx->prof.clear();
    ctx->event_next = 0;
}

// One call = one profile, whatever the number of its chunks: mode 1 starts the call with an empty profile and lets the later chunks
// accumulate like mode 2 (which accumulates across calls); the caller's mode is back on every exit.
struct ProfCall {
    hp3d_ctx* ctx;
    const int saved;
    explicit ProfCall(hp3d_ctx* c) : ctx(c), saved(c->profiling) {
        if (saved != 2) prof_reset(c);
    }
    void chunk(int b0) {
        if (b0 > 0 && saved == 1) ctx->profiling = 2;
    }
    ~ProfCall() { ctx->profiling = saved; }
};

#ifdef HP3D_EMU          // the CPU interpreter has neither page-locked memory nor event flags
int* host_ints_alloc(size_t n) { return (int*)malloc(sizeof(int) * n); }
void host_ints_free(int* p) { free(p); }
hipError_t flag_event_create(hipEvent_t* e) { return hipEventCreate(e); }
#else
int* host_ints_alloc(size_t n) {
    int* p = nullptr;
    return hipHostMalloc((void**)&p, sizeof(int) * n, hipHostMallocDefault) == hipSuccess ? p : nullptr;
}
void host_ints_free(int* p) { hipHostFree(p); }
hipError_t flag_event_create(hipEvent_t* e) { return hipEventCreateWithFlags(e, hipEventDisableTiming); }
#endif

int HostFlags::resize(hp3d_ctx* ctx, size_t n, const char* what) {
    if (h) host_ints_free(h);
    h = host_ints_alloc(n);
    if (!h) HP3D_FAIL(ctx, HP3D_ERR_NOMEM, "%s: host allocation failed", what);
    if (!ev) HIPCHK(ctx, flag_event_create(&ev));
    return 0;
}
int HostFlags::wait(hp3d_ctx* ctx) {
    if (pending) { HIPCHK(ctx, hipEventSynchronize(ev)); pending = false; }
    return 0;
}
int HostFlags::record(hp3d_ctx* ctx) {
    HIPCHK(ctx, hipEventRecord(ev, ctx->stream));
    pending = true;
    return 0;
}
int HostFlags::copy_behind(hp3d_ctx* ctx, const int* d_src, size_t n) {
    HIPCHK(ctx, hipMemcpyAsync(h, d_src, sizeof(int) * n, hipMemcpyDeviceToHost, ctx->stream));
    return record(ctx);
}
void HostFlags::free() {
    if (h) host_ints_free(h);
    if (ev) hipEventDestroy(ev);
    *this = HostFlags();
}

// ---- weight packing ------------------------------------------------------------------------
// wpk[tap][c8][co32][h][n][j] = W_hwio[tap][ref_channel(c8*8+h*4+j)][co32*32+n]   (conv_mfma.hip)
void pack_conv(const ConvL& l, const float* w, const float* b, float* blob) {
    float* wp = blob + l.w_off;
    float* bp = blob + l.b_off;
    const int taps = l.ek * l.ek, C8 = l.cin_pad / 8, CO32 = l.cout_pad / 32;
    memset(wp, 0, sizeof(float) * (size_t)taps * l.cin_pad * l.cout_pad);
    memset(bp, 0, sizeof(float) * l.cout_pad);
    for (int co = 0; co < l.cout; ++co) bp[co] = b[co];
    for (int tap = 0; tap < taps; ++tap)
        for (int e = 0; e < l.cin_pad; ++e) {
            // engine channel e -> (reference tap, reference channel)
            int rtap = tap, rc = -1;
            if (l.mode == 0) {
                rc = (e < l.cin) ? e : -1;
            } else if (l.mode == 1) {            // im2col: e = (r*3+s)*3 + c
                if (e < 27) { rtap = e / 3; rc = e % 3; }
            } else {                             // concat buffer: [encoding 0..127 | scoremap 128..148 | 0]
                if (e < 128) rc = 21 + e;        // reference concat is [scoremap(21), encoding(128)]
                else if (e < 149) rc = e - 128;
            }
            if (rc < 0) continue;
            const int c8 = e >> 3, h = (e >> 2) & 1, j = e & 3;
            const float* src = w + ((size_t)rtap * l.cin + rc) * l.cout;
            for (int co = 0; co < l.cout; ++co) {
                const int co32 = co >> 5, n = co & 31;
                wp[((((size_t)tap * C8 + c8) * CO32 + co32) * 2 + h) * 128 + n * 4 + j] = src[co];
            }
        }
}

// Every float32 section layer l has reserved (reserve_conv), from its HWIO filter w and bias b.
void pack_layer(const ConvL& l, const float* w, const float* b, float* blob) {
    pack_conv(l, w, b, blob);
    if (l.raw_off)          // lift_fused.hip: [cout block of 64][cin4][tap][64], zero rows / columns as padding
        for (int t = 0; t < 9; ++t)
            for (int c = 0; c < l.cin; ++c)
                for (int co = 0; co < l.cout; ++co)
                    blob[l.raw_off + (((size_t)(co >> 6) * l.cin4 + c) * 9 + t) * 64 + (co & 63)] = w[((size_t)t * l.cin + c) * l.cout + co];
    if (l.hwio_off) memcpy(blob + l.hwio_off, w, sizeof(float) * (size_t)9 * l.cin * l.cout);
    if (!(l.ww_off || l.ww2_off || l.ww4_off || l.ww7_off || l.ww4s_off)) return;
    // U = G g G^T in the Winograd kernels' fragment orders
    std::vector<int> cmap(l.cin_pad, -1);
    for (int e = 0; e < l.cin_pad; ++e) {
        if (l.mode == 0) cmap[e] = e < l.cin ? e : -1;
        else if (e < 128) cmap[e] = 21 + e;            // concat buffer [encoding | scoremap | 0] vs reference [scoremap, encoding]
        else if (e < 149) cmap[e] = e - 128;
    }
    if (l.ww_off) wino_pack_weights(w, l.k, l.cin, l.cout, l.cin_pad, l.cout_pad, cmap.data(), blob + l.ww_off);
    if (l.ww2_off) wino2_pack_weights(w, l.k, l.cin, l.cout, l.cin_pad, l.cout_pad, cmap.data(), blob + l.ww2_off);
    if (l.ww4_off) wino4_pack_weights(w, l.k, l.cin, l.cout, l.cin_pad, l.cout_pad, cmap.data(), blob + l.ww4_off);
    if (l.ww7_off) wino7_pack_weights(w, l.cin, l.cout, l.cin_pad, l.cout_pad, cmap.data(), blob + l.ww7_off);
    if (l.ww4s_off) wino4s_pack_weights(w, l.cin, l.cout, l.cin_pad, l.cout_pad, cmap.data(), blob + l.ww4s_off);
}

// half-precision packing: wpk16[tap][Cin/16][Cout/32][h][n][8] = W[tap][ref_channel(16*kb + 8*h + e)][32*co32 + n]
void pack_conv16(const ConvL& l, const float* w, hp3d_f16* blob16) {
    hp3d_f16* wp = blob16 + l.w16_off;
    const int taps = l.ek * l.ek, KB = l.cin_pad16 / 16, CO32 = l.cout_pad / 32;
    for (size_t i = 0; i < (size_t)taps * l.cin_pad16 * l.cout_pad; ++i) wp[i] = (hp3d_f16)0.f;
    for (int tap = 0; tap < taps; ++tap)
        for (int e16 = 0; e16 < l.cin_pad16; ++e16) {
            int rtap = tap, rc = -1;
            if (l.mode == 0) rc = (e16 < l.cin) ? e16 : -1;
            else if (l.mode == 1) { if (e16 < 27) { rtap = e16 / 3; rc = e16 % 3; } }
            else { if (e16 < 128) rc = 21 + e16; else if (e16 < 149) rc = e16 - 128; }
            if (rc < 0) continue;
            const int kb = e16 >> 4, h = (e16 >> 3) & 1, e = e16 & 7;
            const float* src = w + ((size_t)rtap * l.cin + rc) * l.cout;
            for (int co = 0; co < l.cout; ++co)
                wp[((((size_t)tap * KB + kb) * CO32 + (co >> 5)) * 2 + h) * 256 + (co & 31) * 8 + e] = (hp3d_f16)src[co];
        }
}

int find_var(hp3d_ctx* ctx, const std::string& name, const HostVar** out) {
    auto it = ctx->vars.find(name);
    if (it == ctx->vars.end()) return -1;
    *out = &it->second;
    return 0;
}

// the mask growth of an H x W frame runs on the global-scratch kernel (option "mask_grow")
bool mask_grow_global(const hp3d_ctx* ctx, int H, int W) {
    return ctx->mask_grow == 2 || (ctx->mask_grow == 0 && !mask_grow_lds_fits(H, W));
}

// ---- arena ---------------------------------------------------------------------------------
// B images of H x W; `slots` (>= B; 0 = B) crops behind them: the multi-hand calls run K crops per image
int ensure_arena(hp3d_ctx* ctx, int B, int H, int W, int slots = 0) {
    slots = std::max(slots, B);
    const size_t px = std::max((size_t)B * std::max((size_t)H * W, (size_t)256 * 256), (size_t)slots * 256 * 256);
    const size_t act = px * 64;
    if (act > ctx->act_floats) {
        CHK(dev_realloc(ctx, &ctx->bufA, act));
        CHK(dev_realloc(ctx, &ctx->bufB, act));
        ctx->act_floats = act;
    }
    const size_t imgf = (size_t)B * H * W * 3;
    if (imgf > ctx->image_floats) {
        CHK(dev_realloc(ctx, &ctx->d_image, imgf));
        ctx->image_floats = imgf;
    }
    const size_t largef = (size_t)B * H * W * 2;
    if (largef > ctx->large_floats) {
        CHK(dev_realloc(ctx, &ctx->d_large, largef));
        CHK(dev_realloc(ctx, &ctx->d_mask, (size_t)B * H * W));
        ctx->mask_floats = (size_t)B * H * W;
        CHK(dev_realloc(ctx, &ctx->d_fg, (size_t)B * H * W));
        CHK(dev_realloc(ctx, &ctx->d_segsmall, (size_t)B * (H / 8 + 1) * (W / 8 + 1) * 32));
        ctx->large_floats = largef;
    }
    if ((size_t)B * H * W > ctx->det_bytes) {
        CHK(dev_realloc(ctx, &ctx->d_det, (size_t)B * H * W));
        ctx->det_bytes = (size_t)B * H * W;
    }
    if (mask_grow_global(ctx, H, W) && (size_t)B * mask_grow_global_words(H, W) > ctx->mg_words) {
        CHK(dev_realloc(ctx, &ctx->d_mgscratch, (size_t)B * mask_grow_global_words(H, W)));
        ctx->mg_words = (size_t)B * mask_grow_global_words(H, W);
    }
    if (slots > ctx->capB) {
        B = slots;
        CHK(dev_realloc(ctx, &ctx->d_hs, (size_t)B * 2));
        CHK(dev_realloc(ctx, &ctx->d_crop, (size_t)B * 256 * 256 * 3));
        CHK(dev_realloc(ctx, &ctx->d_center, (size_t)B * 2));
        CHK(dev_realloc(ctx, &ctx->d_scale, (size_t)B));
        CHK(dev_realloc(ctx, &ctx->d_cropsize, (size_t)B));
        CHK(dev_realloc(ctx, &ctx->d_kpmap, (size_t)B * 256 * 256 * 21));
        CHK(dev_realloc(ctx, &ctx->d_pooled, (size_t)B * 32 * 32 * 32));
        CHK(dev_realloc(ctx, &ctx->d_coord, (size_t)B * 63));
        CHK(dev_realloc(ctx, &ctx->d_kpimg, (size_t)B * 42));
        CHK(dev_realloc(ctx, &ctx->d_kpcrop, (size_t)B * 42));
        CHK(dev_realloc(ctx, &ctx->d_can, (size_t)B * 63));
        CHK(dev_realloc(ctx, &ctx->d_rot, (size_t)B * 9));
        CHK(dev_realloc(ctx, &ctx->d_u, (size_t)B * 4));
        CHK(dev_realloc(ctx, &ctx->d_fc1, (size_t)B * 512));
        CHK(dev_realloc(ctx, &ctx->d_fc2, (size_t)B * 512));
        CHK(dev_realloc(ctx, &ctx->d_fcpart, std::max((size_t)B * 17 * 512 + (size_t)B * 33 * 256, (size_t)B * 16 * 18 * 256)));      // (FC slices; conv_s2_gemm: 18 slices x 16 B rows x 256)
        CHK(dev_realloc(ctx, &ctx->d_seed, (size_t)B * 2));
        CHK(dev_realloc(ctx, &ctx->d_valid, (size_t)B));
        CHK(dev_realloc(ctx, &ctx->d_area, (size_t)B));
        CHK(dev_realloc(ctx, &ctx->d_keys, (size_t)B));
        CHK(dev_realloc(ctx, &ctx->d_keepc, (size_t)B * 2));
        CHK(dev_realloc(ctx, &ctx->d_keeps, (size_t)B));
        ctx->capB = B;
        ctx->sideB = B;
    }
    return 0;
}

// concat / scoremap buffers depend on the PoseNet input size (h/8 x w/8)
int ensure_pose_bufs(hp3d_ctx* ctx, int B, int hs, int ws) {
    const size_t px = (size_t)B * hs * ws;
    if (px > ctx->pose_px || !ctx->d_concat) {
        CHK(dev_realloc(ctx, &ctx->d_concat, px * 160));
        for (int i = 0; i < 3; ++i) CHK(dev_realloc(ctx, &ctx->d_sm[i], px * 32));
        CHK(dev_realloc(ctx, &ctx->d_concat16, px * 192));
        HIPCHK(ctx, hipMemsetAsync(ctx->d_concat16, 0, px * 192 * sizeof(hp3d_f16), ctx->stream));
        ctx->pose_px = px;
    }
    return 0;
}

void same_pad(int in, int k, int stride, int* out, int* before) {
    *out = (in + stride - 1) / stride;
    int total = (*out - 1) * stride + k - in;
    if (total < 0) total = 0;
    *before = total / 2;
}

// Which Winograd kernel a layer takes when both can run it (option "wino2" = "auto"): a small cost model in units of one CU-time of
// conv_wino.hip's item-step (32 tiles x 128 couts x 32 channels), fitted to per-layer timings of both kernels at B = 1 ... 32
// (profiles/r03_tuning_notes.md).  conv_wino.hip walks ceil(items / CUs) rounds of whole items; conv_wino2.hip's items are a quarter
// of that work each, two run per CU, so its time is the balanced share plus one small item of tail -- it wins where the coarse rounds
// quantise badly (300 items on 256 CUs) and at small batches, and loses ~7 % on long filled launches (twice the window traffic and
// input-transform work per MFMA).  `old_nt` / `old_ks`: conv_wino_eligible's answer for the same layer (0: it would not run).
// conv_wino.hip's time for a layer (`old_nt` / `old_ks` as above).  frac_rounds: the last round of items counts fractionally
// (wino4_auto with the second stream live); otherwise whole rounds.
double wino_cost(int k, int cin_pad, int cout_pad, int Ho, int Wo, int B, int old_nt, int old_ks, bool frac_rounds) {
    const double cus = hp3d_num_cus(), reduce_cost = 0.7;
    const long tiles = (long)B * ((Ho + 1) / 2) * ((Wo + 1) / 2);
    const int nsub = k == 7 ? 9 : 1;
    const long items1 = (tiles + old_nt - 1) / old_nt * (cout_pad / (old_nt == 32 ? 128 : 64));
    const int S1 = nsub * cin_pad / (old_nt == 32 ? 32 : 16);
    const double w1 = old_nt == 32 ? 1.0 : 0.5;
    const double rounds = frac_rounds ? std::max(1.0, items1 / cus) : std::ceil(items1 / cus);
    return old_ks > 1 ? std::ceil((double)S1 / old_ks) * w1 * std::max(1.0, items1 * old_ks / cus) + reduce_cost : rounds * S1 * w1;
}
// conv_wino2.hip's time for a layer split `ks2` ways
double wino2_cost(int k, int cin_pad, int cout_pad, int Ho, int Wo, int B, int ks2) {
    const double cus = hp3d_num_cus(), reduce_cost = 0.7, c2 = 1.07;
    const long tiles = (long)B * ((Ho + 1) / 2) * ((Wo + 1) / 2);
    const int nsub = k == 7 ? 9 : 1;
    const long items2 = (tiles + 31) / 32 * (cout_pad / 64);
    const int S2 = nsub * cin_pad / 16;
    return ks2 > 1 ? c2 * (std::ceil((double)S2 / ks2) * 0.25 * std::max(1.0, items2 * ks2 / cus)) + reduce_cost
                   : c2 * (items2 * S2 * 0.25 / cus + S2 * 0.125);
}
bool wino2_auto(int k, int cin_pad, int cout_pad, int Ho, int Wo, int B, int old_nt, int old_ks, int ks2, bool two_streams) {
    if ((long)B * Ho * Wo < 512) return false;              // 16 x 16 maps and below: one direct launch beats split + reduce
    if (!old_nt) return Ho * Wo >= 900 && cin_pad >= 64;      // trunk layers conv_wino.hip cannot fill; the lifting nets' 16 x 16 / 8 x 8 maps stay direct
    const double t_old = wino_cost(k, cin_pad, cout_pad, Ho, Wo, B, old_nt, old_ks, false);
    const double t_new = wino2_cost(k, cin_pad, cout_pad, Ho, Wo, B, ks2);
    // with a second stream on the GPU the other half's kernels fill conv_wino.hip's tail rounds anyway (measured: B = 16 as 8 + 8
    // loses 2 % when its filled layers switch): only under-filled launches are candidates then
    if (two_streams && old_ks <= 1) return false;
    return t_new < 0.97 * t_old;
}

// Which layers take the F(4x4,3x3) kernel (option "wino4" = "auto": both trunks; "pose": PoseNet2D only).  Numerics: end to end the larger
// Winograd tile moves PoseNet2D's heat-maps by 5e-6 (gate 1e-3) and the 3-D keypoints by 3e-6 (gate 1e-4).  HandSegNet's score map
// feeds a THRESHOLD (the hand mask), where any change of summation order flips pixels whose two logits are equal to rounding: against
// the all-direct-kernel run, 24 of 512 synthetic images differ in at least one mask pixel with F(2x2,3x3) and 35 with F(4x4,3x3); the
// crop box and the keypoints (1e-4) agree on all 512 either way (scripts/mask_flip_rate.py, profiles/r03_tuning_notes.md section 7).
// Speed: the cost model below, fitted to per-layer timings of the three Winograd kernels at B = 1 ... 32.
// what option "wino4" = "auto" means: both trunks by the cost model below (-2).  HP3D_WINO4_AUTO=pose in the environment keeps
// HandSegNet on F(2x2,3x3) (-1; the same as option "wino4" = "pose") -- for A/B runs of whole test suites.
static int wino4_default() {
    const char* e = getenv("HP3D_WINO4_AUTO");
    return (e && !strcmp(e, "pose")) ? -1 : -2;
}
bool wino4_auto(int mode, bool posenet, int k, int cin_pad, int cout_pad, int Ho, int Wo, int B, int ks4, int old_nt, int old_ks, int ks2,
                bool two_streams) {
    if (mode == -1 && !posenet) return false;              // -1 = option "pose": PoseNet2D only; -2 = "auto": both trunks
    if ((long)B * Ho * Wo < 1024) return false;
    const double cus = hp3d_num_cus(), reduce_cost = 0.7;
    const int nsub = k == 7 ? 9 : 1;
    // units: one conv_wino.hip item-step (32 F(2x2) tiles x 128 couts x 32 channels).  A conv_wino4 item-step (32 F(4x4) tiles x 64
    // couts x 16 channels) covers the same amount of convolution and was measured at 0.72-0.78 of its time on filled launches
    // (7x7 layers 0.85: their split partial sums go through a reduce launch).  With the second stream live the other half's kernels
    // fill tail rounds, so rounds count fractionally.
    auto rounds = [&](double items) { return two_streams ? std::max(1.0, items / cus) : std::ceil(items / cus); };
    double t_best = old_nt ? wino_cost(k, cin_pad, cout_pad, Ho, Wo, B, old_nt, old_ks, two_streams) : 1e30;
    t_best = std::min(t_best, wino2_cost(k, cin_pad, cout_pad, Ho, Wo, B, ks2));
    const long tiles4 = (long)B * ((Ho + 3) / 4) * ((Wo + 3) / 4);
    const long items4 = (tiles4 + 31) / 32 * (cout_pad / 64);
    const int S4 = nsub * cin_pad / 16;
    if (ks4 > 1 && (S4 + ks4 - 1) / ks4 < 8) return false;      // short split items are all prologue / epilogue (measured: B <= 2 loses)
    const double c4 = k == 7 ? 0.85 : 0.76;
    double t4 = ks4 > 1 ? c4 * std::ceil((double)S4 / ks4) * std::max(1.0, items4 * ks4 / cus) + reduce_cost : c4 * rounds((double)items4) * S4;
    // A 3x3 launch's last, under-filled round runs as tail pieces (conv_wino4_tail_plan): q steps instead of a whole round of S4, + the
    // pieces' epilogues and the tail reduce launch (~2 units).  Round 5: the model above charged a whole round and sent B = 12 / 24 layers with
    // 1.2-1.5 rounds of items to the F(2x2,3x3) kernels (PoseNet2D conv4_2 at B = 24: 0.416 ms there against 0.352 for THIRTY-TWO images here).
    // (Rounds 4-5 applied this to PoseNet2D only: HandSegNet's logits feed the mask threshold, and the reference-code fixtures demanded bit-equal
    // masks of noise maps whose knife-edge pixels move with ANY change of summation order -- a test fixture was choosing kernels.  Round 6: the
    // fixtures carry the reference run's knife-edge pixels and the tests tell such a flip from a defect (tests/test_gpu_reference_fixtures.py:
    // _mask_gate), so both trunks take the plan the model prices: +5-12 % at B = 8 ... 24, throughput monotonic in B again.)
    if (k == 3 && ks4 <= 1 && !two_streams) {
        int tail_items = 0;
        const int q = conv_wino4_tail_plan(cin_pad, cout_pad, Ho, Wo, B, &tail_items);
        if (q > 0 && tail_items > 0) t4 = std::min(t4, c4 * (std::floor(items4 / cus) * S4 + q) + 2.0);
    }
    return t4 < 0.97 * t_best;
}

static int wino2_ks_probe(hp3d_ctx* ctx, const ConvL& l, int Ho, int Wo, int B, int in_cs, int out_cs, int pool) {
    int ks = 1;
    (void)conv_wino2_eligible(l.k, l.stride, l.cin_pad, l.cout_pad, Ho, Wo, B, in_cs, out_cs, pool, ctx->wino_splitk ? &ks : nullptr);
    return ks;
}

int kid_sync_state(hp3d_ctx* ctx);

// Work forked onto the child context's stream (after kid_sync_state): the child's stream starts after everything already queued on
// this context's (inputs produced there), and whatever happens after the fork, the join is recorded and waited for on EVERY exit path
// -- this context's stream must not run ahead of (and hp3d_sync / hp3d_dev_free / hp3d_destroy must cover) what was enqueued on the
// child's.  two_streams: the two halves of a whole-path call (two_streams_live is set on both contexts until the join).
struct KidFork {
    hp3d_ctx* ctx = nullptr;
    bool two_streams = false;
    int fork(hp3d_ctx* c, bool two = false) {
#ifndef HP3D_EMU
        HIPCHK(c, hipEventRecord(c->ev_fork, c->stream));
        HIPCHK(c, hipStreamWaitEvent(c->kid->stream, c->ev_fork, 0));
        ctx = c;
        two_streams = two;
        if (two) c->two_streams_live = c->kid->two_streams_live = true;
        return 0;
#else
        HP3D_FAIL(c, HP3D_ERR_UNSUPPORTED, "no second stream in the CPU interpreter build");
#endif
    }
    ~KidFork() {
#ifndef HP3D_EMU
        if (!ctx) return;
        hp3d_ctx* k = ctx->kid;
        if (two_streams) ctx->two_streams_live = k->two_streams_live = false;
        if (hipEventRecord(ctx->ev_join, k->stream) == hipSuccess) (void)hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0);
        else (void)hipStreamSynchronize(k->stream);
#endif
    }
};

// ---- one convolution layer -------------------------------------------------------------------
static int wino7_ks_override(const hp3d_ctx* ctx, int ks, int cin_pad, long out_floats) {        // option "wino7_ksplit"
    if (ctx->wino7_ksplit <= 0 || !ctx->wino_splitk) return ks;
    ks = std::min(ctx->wino7_ksplit, cin_pad / 16);
    return (ks >= 2 && ks * out_floats * 4 < (1L << 31)) ? ks : 1;
}

// The ConvParams fields every form of a layer sets; each form then sets what differs (tiles, ksplit, nsub, im2col, f16, partial).
ConvParams conv_params(const float* in, const float* wpk, const float* bias, float* out, int B, int H, int W, int Ho, int Wo, int Cin, int in_cs,
                       int Cout, int out_cs, int cout_store, int pad_t, int pad_l, int act) {
    ConvParams p;
    p.in = in; p.wpk = wpk; p.bias = bias; p.out = out;
    p.B = B; p.H = H; p.W = W; p.Ho = Ho; p.Wo = Wo;
    p.Cin = Cin; p.in_cs = in_cs; p.Cout = Cout; p.out_cs = out_cs; p.cout_store = cout_store;
    p.pad_t = pad_t; p.pad_l = pad_l; p.act = act;
    p.tiles_x = 0; p.tiles_y = 0; p.ksplit = 1; p.partial = nullptr; p.f16 = 0; p.out_f32 = 0; p.im2col = 0; p.nsub = 1;
    return p;
}

// Grows the scratch of split-K partial sums / tail pieces (launches still queued may read the old buffer: synchronise first).
int ensure_col(hp3d_ctx* ctx, size_t floats) {
    if (floats > ctx->col_floats) {
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        CHK(dev_realloc(ctx, &ctx->col, floats));
        ctx->col_floats = floats;
    }
    return 0;
}

// The reduce behind a channel-split launch: ctx->col = [ks][B*Ho*Wo][cout_pad] raw sums -> bias + activation (+ the layer's 2x2
// max-pool) -> out.  profile = false: no profile row (conv_mfma's reduce never had one).
void splitk_reduce(hp3d_ctx* ctx, const ConvL& l, const float* bias, int ks, int B, int Ho, int Wo, int pool, float* out, int out_cs, bool profile = true) {
    ProfScope ps(ctx, l.name, !profile ? nullptr : pool ? "conv_splitk_reduce_pool" : "conv_splitk_reduce", 0.0, 4.0 * (ks + 1) * B * Ho * Wo * l.cout_pad);
    ++ctx->conv_splitk_reduce_launches;
    if (pool)
        conv_splitk_reduce_pool_launch(ctx->col, ks, B, Ho, Wo, l.cout_pad, bias, l.relu, out, out_cs, std::min(l.cout_pad, out_cs), ctx->stream);
    else
        conv_splitk_reduce_launch(ctx->col, ks, (long)B * Ho * Wo, l.cout_pad, bias, l.relu, out, out_cs, std::min(l.cout_pad, out_cs), ctx->stream);
}

// The Winograd kernel a layer takes, decided before anything is launched.
enum WinoKind { WINO_NONE, WINO7, WINO4S, WINO4, WINO2, WINO };
struct WinoPick {
    WinoKind kind = WINO_NONE;
    size_t w_off = 0;          // its packed filters in the blob
    int ks = 1;                // channel splits (> 1: raw partial sums to ctx->col, then splitk_reduce)
    std::string kernel;        // the profile row's kernel name
};

WinoPick pick_wino(hp3d_ctx* ctx, const ConvL& l, int in_cs, int out_cs, int B, int Ho, int Wo, int pool, int f16) {
    if (!ctx->use_wino || f16) return {};
    auto take = [&](WinoKind kind, size_t off, int ks, const char* stem) {
        return WinoPick{kind, off, ks, std::string(stem) + (l.k == 7 ? (ks > 1 ? "_as7x7_splitk" : "_as7x7") : ks > 1 ? "_splitk" : pool ? "_pool" : "")};
    };
    int wino_ks = 1, wino2_ks = 1, wino4_ks = 1, ks7 = 1;
    const int old_nt = l.ww_off ? conv_wino_eligible(ctx->use_wino, l.k, l.stride, l.cin_pad, l.cout_pad, Ho, Wo, B, in_cs, out_cs, pool,
                                                     ctx->wino_splitk ? &wino_ks : nullptr) : 0;
    // 7x7 layers (PoseNet2D's refinement units): Winograd F(4x4,4x4) over the filter's four 4x4-tap blocks when the launch fills the chip
    // (one work item = a 4x4 tile block x 64 couts, no channel split: 160 of 256 CUs busy already beats the split nine-block form + its reduce)
    // (under-filled launches -- small batches -- split the 16-channel chunks over workgroups and add the raw sums in a reduce launch, like the other
    //  Winograd kernels: option "wino_splitk")
    long items7 = 0;
    if (ctx->use_wino7 && l.ww7_off && !pool && !ctx->conv_naive &&
        conv_wino7_eligible(l.k, l.stride, l.cin_pad, l.cout_pad, Ho, Wo, B, in_cs, out_cs, &items7, ctx->wino_splitk ? &ks7 : nullptr)) {
        ks7 = wino7_ks_override(ctx, ks7, l.cin_pad, (long)B * Ho * Wo * l.cout_pad);
        if (ctx->use_wino7 == 1 || items7 >= (long)hp3d_num_cus() * 5 / 8 || (ks7 > 1 && ctx->use_wino7 == -1 && !ctx->two_streams_live))
            return take(WINO7, l.ww7_off, ks7, "conv_wino7_f4x4_4x4");
    }
    const bool take4 = ctx->use_wino4 && l.ww4_off && !ctx->conv_naive &&
        conv_wino4_eligible(l.k, l.stride, l.cin_pad, l.cout_pad, Ho, Wo, B, in_cs, out_cs, pool, ctx->wino_splitk ? &wino4_ks : nullptr) &&
        (ctx->use_wino4 == 1 ||
         (ctx->use_wino4 < 0 && wino4_auto(ctx->use_wino4, l.net == NET_POSE, l.k, l.cin_pad, l.cout_pad, Ho, Wo, B, wino4_ks, old_nt, wino_ks,
                                           wino2_ks_probe(ctx, l, Ho, Wo, B, in_cs, out_cs, pool), ctx->two_streams_live)));
    // round 6: the filled 3x3 launches with Cin >= 128 on the bf16 matrix pipe with split operands (conv_wino4s.hip), option "wino4_split"
    int filled4s = 0;
    if (ctx->use_wino4s && l.ww4s_off && !ctx->conv_naive && l.k == 3 &&
        conv_wino4s_eligible(l.k, l.stride, l.cin_pad, l.cout_pad, Ho, Wo, B, in_cs, out_cs, pool, &filled4s) &&
        (ctx->use_wino4s == 1 || (take4 && wino4_ks <= 1 && filled4s)))
        return take(WINO4S, l.ww4s_off, 1, "conv_wino4s_f4x4_3x3_bf16x3");
    if (take4) return take(WINO4, l.ww4_off, wino4_ks, "conv_wino4_f4x4_3x3");
    if (ctx->use_wino2 && l.ww2_off && !ctx->conv_naive &&
        conv_wino2_eligible(l.k, l.stride, l.cin_pad, l.cout_pad, Ho, Wo, B, in_cs, out_cs, pool, ctx->wino_splitk ? &wino2_ks : nullptr) &&
        (ctx->use_wino2 == 1 || wino2_auto(l.k, l.cin_pad, l.cout_pad, Ho, Wo, B, old_nt, wino_ks, wino2_ks, ctx->two_streams_live)))
        return take(WINO2, l.ww2_off, wino2_ks, "conv_wino2_f2x2_3x3");
    if (old_nt) return take(WINO, l.ww_off, wino_ks, "conv_wino_f2x2_3x3");
    return {};
}

// Launches the Winograd form `w` of layer l; p = the layer's common parameters with w's filters.  All forms share one protocol: a
// channel split writes raw partial sums at conv resolution to ctx->col and the pool (if any) happens in the reduce.
int run_wino(hp3d_ctx* ctx, const ConvL& l, const WinoPick& w, ConvParams p, int pool, double flops, double bytes) {
    float* const out = p.out;
    const int out_cs = p.out_cs, B = p.B, Ho = p.Ho, Wo = p.Wo;
    p.ksplit = w.ks;
    p.nsub = w.kind == WINO7 ? 4 : l.k == 7 ? 9 : 1;
    if (w.kind == WINO) { p.tiles_x = (Wo + 15) / 16; p.tiles_y = (Ho + 7) / 8; }
    if (w.ks > 1) {        // under-filled chip: channel steps split over workgroups
        CHK(ensure_col(ctx, (size_t)w.ks * B * Ho * Wo * l.cout_pad));
        p.out = ctx->col; p.out_cs = l.cout_pad; p.cout_store = l.cout_pad;
    } else if ((w.kind == WINO4 || w.kind == WINO4S) && l.k == 3 && ctx->w4_tail && conv_wino4_tail_plan(l.cin_pad, l.cout_pad, Ho, Wo, B, nullptr) > 0) {
        // an under-filled last round of items runs as channel slices, one piece per CU (conv_wino4.hip, TAIL): scratch for the raw sums
        CHK(ensure_col(ctx, w.kind == WINO4 ? conv_wino4_tail_floats() : conv_wino4s_tail_floats()));
        p.partial = ctx->col; p.partial_cap = ctx->col_floats;
    }
    {
        ProfScope ps(ctx, l.name, w.kernel.c_str(), flops, bytes);
        const int lpool = w.ks > 1 ? 0 : pool;
        // (the F(4x4,3x3) launchers answer 1 when the last round really ran as tail pieces: the counters are the tests' proof)
        int lr;
        switch (w.kind) {
        case WINO7:
            if (conv_wino7_launch(p, ctx->stream)) HP3D_FAIL(ctx, HP3D_ERR_ARG, "winograd conv (F(4x4,4x4)): launch refused");
            ++ctx->conv_wino7_launches;
            ctx->conv_wino7_split_launches += w.ks > 1;
            break;
        case WINO4S:
            if ((lr = conv_wino4s_launch(p, lpool, ctx->stream)) < 0) HP3D_FAIL(ctx, HP3D_ERR_ARG, "winograd conv (F(4x4,3x3), split operands): launch refused");
            ++ctx->conv_wino4s_launches;
            ctx->conv_wino4s_tail_launches += lr == 1;
            break;
        case WINO4:
            if ((lr = conv_wino4_launch(p, lpool, ctx->stream)) < 0) HP3D_FAIL(ctx, HP3D_ERR_ARG, "winograd conv (F(4x4,3x3)): launch refused");
            ++ctx->conv_wino4_launches;
            ctx->conv_wino4_tail_launches += lr == 1;
            break;
        case WINO2:
            if (conv_wino2_launch(p, lpool, ctx->stream) < 0) HP3D_FAIL(ctx, HP3D_ERR_ARG, "winograd conv (2 workgroups per CU): launch refused");
            ++ctx->conv_wino2_launches;
            break;
        default:
            if (conv_wino_launch(p, lpool, ctx->stream)) HP3D_FAIL(ctx, HP3D_ERR_ARG, "winograd conv: tensor exceeds 32-bit offsets");
            ++ctx->conv_wino_launches;
        }
    }
    if (w.ks > 1) splitk_reduce(ctx, l, p.bias, w.ks, B, Ho, Wo, pool, out, out_cs);
    return 0;
}

// conv1_1 on its own kernel (conv_first.hip); p = the layer's parameters
int run_conv_first(hp3d_ctx* ctx, const ConvL& l, const ConvParams& p, double flops, double bytes) {
    const size_t px = (size_t)p.B * p.H * p.W;
    // A COLD input image (the caller's device buffer, an upload: not written by the kernel in front of this one) costs this
    // store-bound kernel a third of its rate -- its gathers run one tile ahead, an HBM miss takes longer than a tile (round 5: 3.5
    // TB/s in the pipeline against 4.8 standalone and for PoseNet2D's freshly written crop).  Streaming the image once through the
    // memory-side cache first (13 us for 39 MB) takes B = 32 at 320 x 320 from 0.253 to 0.175 ms (5.0 TB/s = 0.63 of the HBM spec).
    const size_t img_bytes = px * 12;
    // The pass runs on the child context's stream BESIDE the convolution (it is ahead of the gathers after the first few tiles and
    // needs 16 registers per wave next to the convolution's 3 x 160): its 13 us disappear; in this stream when there is no second one.
    KidFork beside;            // (joined when this function returns: the call's completion covers the read pass)
    if (l.net && ctx->d_keys && (ctx->first_touch == 1 || (ctx->first_touch < 0 && !ctx->trunk_input_hot && img_bytes >= (8u << 20) && img_bytes <= (128u << 20)))) {
        if (ctx->first_touch_beside && !ctx->use_graph && !ctx->shared_weights && !ctx->two_streams_live && kid_sync_state(ctx) == 0) {
            CHK(beside.fork(ctx));          // (whatever produced the image on this stream comes first)
            touch_launch(p.in, px * 3, (float*)ctx->d_keys, ctx->kid->stream);
        } else {
            ProfScope pt(ctx, l.name, "conv_first_touch", 0.0, 0.0);
            touch_launch(p.in, px * 3, (float*)ctx->d_keys, ctx->stream);
        }
        ++ctx->first_touch_launches;
    }
    {
        ProfScope ps(ctx, l.name, p.f16 ? "conv_first_3x3_c3_f16" : "conv_first_3x3_c3", flops, bytes);
        conv_first_launch(p, ctx->stream, ctx->first_balanced);
    }
    ++ctx->conv_first_launches;
    return 0;
}

// Where a layer's filters are: the blobs its offsets refer to, and its raw HWIO filter for conv_impl=naive.
struct ConvW {
    const float* f32;
    const hp3d_f16* f16;
    const float* hwio;
};

// in: [B,H,W,in_cs] (engine channels start at `in`), out: [B,Ho',Wo',out_cs] channel 0 at `out`.
// f16 = 1 (trunk nets after hp3d_finalize_weights(dtype=1)): `in` / `out` hold halves (except the raw image of
// conv1_1 and out_f32 heads); in_cs / out_cs are then counted in ELEMENTS of the respective tensor.
int run_conv(hp3d_ctx* ctx, const ConvW& wts, const ConvL& l, const float* in, int in_cs, int B, int H, int W, float* out, int out_cs,
             int pool, int* Ho_out, int* Wo_out, int f16 = 0, int out_f32 = 0) {
    const float* const bias = wts.f32 + l.b_off;
    int Ho, Wo, pt, pl;
    const int k = l.ek;
    same_pad(H, k, l.stride, &Ho, &pt);
    same_pad(W, k, l.stride, &Wo, &pl);
    const double flops = 2.0 * l.k * l.k * l.cin * l.cout * (double)Ho * Wo * B;
    const double bytes = (f16 ? 2.0 : 4.0) * ((double)B * H * W * l.cin + (double)l.k * l.k * l.cin * l.cout + l.cout +
                                (double)B * (pool ? (Ho / 2) * (Wo / 2) : Ho * Wo) * l.cout);
    if (l.hwio_off && ctx->tiny_gemm && !f16 && !pool && !ctx->conv_naive && l.stride == 2 && l.k == 3 && H == 8 && W == 8 && in_cs == l.cin && out_cs == l.cout) {
        // the last stride-2 layer of a lifting tower: 16 output pixels per image -- a split-K GEMM over them (glue.hip: conv_s2_gemm_launch)
        ProfScope ps(ctx, l.name, "conv_s2_gemm", flops, bytes);
        conv_s2_gemm_launch(in, B, 8, l.cin, wts.f32 + l.hwio_off, bias, l.cout, l.relu, out, ctx->d_fcpart, ctx->stream);
        ++ctx->conv_s2_gemm_launches;
        HIPCHK(ctx, hipGetLastError());
        if (Ho_out) *Ho_out = Ho;
        if (Wo_out) *Wo_out = Wo;
        return 0;
    }
    const WinoPick wp = pick_wino(ctx, l, in_cs, out_cs, B, Ho, Wo, pool, f16);
    if (wp.kind != WINO_NONE) {
        CHK(run_wino(ctx, l, wp, conv_params(in, wts.f32 + wp.w_off, bias, out, B, H, W, Ho, Wo, l.cin_pad, in_cs, l.cout_pad,
                                              out_cs, std::min(l.cout_pad, out_cs), pt, pl, l.relu), pool, flops, bytes));
    } else if (l.mode == 1 && !pool && !out_f32 && ctx->use_first && !ctx->conv_naive &&
               conv_first_eligible(l.k, l.stride, l.cin, l.cout, B, H, W, out_cs, f16)) {
        ConvParams p = conv_params(in, wts.f32 + l.w_off, bias, out, B, H, W, Ho, Wo, 3, 3, 64, out_cs, 64, pt, pl, l.relu);
        p.im2col = 1; p.f16 = f16;
        CHK(run_conv_first(ctx, l, p, flops, bytes));
    } else if (f16 && ctx->use_h16 && !ctx->conv_naive &&
               ((l.mode == 0 && l.k == 3) || (ctx->h16_k7k1 && ((l.k == 7 && (l.mode == 0 || l.mode == 2)) || (l.k == 1 && l.mode == 0)))) &&
               conv_h16_eligible(ctx->use_h16, l.k, l.stride, l.cin_pad16 / 2, l.cout_pad, Ho, Wo, B, out_f32, out_cs) &&
               ((uintptr_t)out & 15) == 0 && !(pool && ((Ho | Wo) & 1))) {
        ConvParams p = conv_params(in, (const float*)(wts.f16 + l.w16_off), bias, out, B, H, W, Ho, Wo, l.cin_pad16 / 2, in_cs / 2,
                                   l.cout_pad, out_cs, std::min(l.cout_pad, out_cs), pt, pl, l.relu);
        p.f16 = 1;
        ProfScope ps(ctx, l.name, l.k == 7 ? "conv_h16_7x7" : l.k == 1 ? "conv_h16_1x1" : pool ? "conv_h16_3x3_pool" : "conv_h16_3x3", flops, bytes);
        ++ctx->conv_h16_launches;
        if (conv_h16_launch(p, pool, ctx->stream)) HP3D_FAIL(ctx, HP3D_ERR_UNSUPPORTED, "conv_h16 launch failed for %s", l.name.c_str());
    } else if (ctx->conv_naive && l.mode == 0 && !pool && !f16) {
        ProfScope ps(ctx, l.name, "conv_naive", flops, bytes);
        conv_naive_launch(in, B, H, W, l.cin, in_cs, wts.hwio, bias, l.k, l.stride, l.cout,
                          l.relu, out, out_cs, Ho, Wo, pt, pl, ctx->stream);
    } else {
        ConvPlan plan;
        const int cin_units = f16 ? l.cin_pad16 / 2 : l.cin_pad;       // 4-byte channel units the kernel iterates
        if (conv_mfma_plan(k, l.stride, Ho, Wo, cin_units, l.cout_pad, pool, B, &plan) != 0)
            HP3D_FAIL(ctx, HP3D_ERR_UNSUPPORTED, "no conv_mfma variant for %s (k=%d s=%d)", l.name.c_str(), k, l.stride);
        if (l.mode == 1 || (f16 && !out_f32)) plan.ksplit = 1;          // split-K partials are float32
        if (plan.ksplit > 1) CHK(ensure_col(ctx, (size_t)plan.ksplit * B * Ho * Wo * l.cout_pad));
        ConvParams p = conv_params(in, f16 ? (const float*)(wts.f16 + l.w16_off) : wts.f32 + l.w_off, bias, out, B, H, W, Ho, Wo,
                                   cin_units, (f16 && l.mode != 1) ? in_cs / 2 : in_cs, l.cout_pad, out_cs, std::min(l.cout_pad, out_cs), pt, pl, l.relu);
        p.f16 = f16; p.out_f32 = out_f32;
        p.tiles_x = (Wo + plan.tw - 1) / plan.tw; p.tiles_y = (Ho + plan.th - 1) / plan.th;
        p.im2col = (l.mode == 1);
        p.ksplit = plan.ksplit; p.partial = ctx->col;
        std::string kname = conv_mfma_variant_name(k, l.stride, pool, plan);
        if (f16) kname += "_f16";
        ProfScope ps(ctx, l.name, kname.c_str(), flops, bytes);
        if (conv_mfma_launch(p, k, l.stride, pool, plan, ctx->stream) != 0)
            HP3D_FAIL(ctx, HP3D_ERR_UNSUPPORTED, "conv_mfma launch failed for %s", l.name.c_str());
        ++ctx->conv_mfma_launches;
        if (plan.ksplit > 1) splitk_reduce(ctx, l, p.bias, plan.ksplit, B, Ho, Wo, pool, out, out_cs, false);      // (conv_mfma_plan splits no pooled layer)
    }
    HIPCHK(ctx, hipGetLastError());
    if (Ho_out) *Ho_out = pool ? Ho / 2 : Ho;
    if (Wo_out) *Wo_out = pool ? Wo / 2 : Wo;
    return 0;
}

// A layer of the networks: its filters are in the context's blobs
int run_conv(hp3d_ctx* ctx, const ConvL& l, const float* in, int in_cs, int B, int H, int W, float* out, int out_cs,
             int pool, int* Ho_out, int* Wo_out, int f16 = 0, int out_f32 = 0) {
    const float* hwio = nullptr;
    if (ctx->conv_naive) {
        auto it = ctx->naive_w.find(l.name);
        if (it != ctx->naive_w.end()) hwio = it->second;
    }
    return run_conv(ctx, ConvW{ctx->blob, ctx->blob16, hwio}, l, in, in_cs, B, H, W, out, out_cs, pool, Ho_out, Wo_out, f16, out_f32);
}

const ConvL& CL(hp3d_ctx* ctx, const char* name) { return ctx->T.conv[ctx->T.conv_idx.at(name)]; }
const FcL& FL(hp3d_ctx* ctx, const char* name) { return ctx->T.fc[ctx->T.fc_idx.at(name)]; }

// Two 1x1 layers as one launch (conv_pw2.hip): l1 = 128 -> H (a multiple of 128), l2 = H -> at most 32 couts, float32 mode, enough pixels to fill
// the chip (64 pixels per workgroup, two workgroups per CU).  Returns 1 if it ran, 0 if the shapes / options do not allow it (the caller
// then runs the two layers one by one).
int run_pw2(hp3d_ctx* ctx, const ConvL& l1, const ConvL& l2, const float* in, int in_cs, int B, int h, int w, float* out, int out_cs) {
    const long npix = (long)B * h * w;
    if (!ctx->use_pw2 || ctx->prec || ctx->conv_naive || l1.k != 1 || l2.k != 1 || l1.stride != 1 || l2.stride != 1 || l1.mode != 0 || l2.mode != 0 ||
        l2.cin_pad != l1.cout_pad || (ctx->use_pw2 == 1 && npix < 64L * hp3d_num_cus()) ||
        !conv_pw2_eligible(l1.cin_pad, l1.cout_pad, l2.cout_pad, npix, in_cs, out_cs) || (in_cs & 3) || ((uintptr_t)in & 15))
        return 0;
    Pw2Params p;
    p.in = in; p.in_cs = in_cs; p.npix = npix;
    p.w1 = ctx->blob + l1.w_off; p.b1 = ctx->blob + l1.b_off; p.H = l1.cout_pad; p.act1 = l1.relu;
    p.w2 = ctx->blob + l2.w_off; p.b2 = ctx->blob + l2.b_off; p.act2 = l2.relu;
    p.out = out; p.out_cs = out_cs; p.cout_store = std::min(l2.cout_pad, out_cs);
    const double flops = 2.0 * npix * ((double)l1.cin * l1.cout + (double)l2.cin * l2.cout);
    const double bytes = 4.0 * (npix * ((double)l1.cin + l2.cout) + (double)l1.cin * l1.cout + (double)l2.cin * l2.cout);
    ProfScope ps(ctx, l1.name + "+" + l2.name.substr(l2.name.find('/') + 1), "conv_pw2_1x1_1x1", flops, bytes);
    if (conv_pw2_launch(p, ctx->stream)) HP3D_FAIL(ctx, HP3D_ERR_ARG, "conv_pw2: launch refused for %s", l1.name.c_str());
    ++ctx->conv_pw2_launches;
    HIPCHK(ctx, hipGetLastError());
    return 1;
}

// Half-precision trunks: conv1_1 (3 -> 64) + conv1_2 (64 -> 64) + 2x2 max-pool as ONE launch of conv_h16.hip's fused form
// (conv1_1's activation never reaches HBM).  Returns 1 if it ran, 0 if the shape / options do not allow it.
// wts: the blobs the two layers' offsets refer to; f16: the caller's precision (the fused form exists in half precision only).
int run_fused12(hp3d_ctx* ctx, const ConvW& wts, int f16, const ConvL& l1, const ConvL& l2, const float* image, int B, int H, int W, float* out,
                int* oh, int* ow) {
    if (!f16 || !ctx->use_h16 || !ctx->fuse12 || ctx->conv_naive || l1.mode != 1 || l2.mode != 0 || l1.cout != 64 || l2.cout != 64 ||
        !l1.relu || !l2.relu || ((H | W) & 1) || ((uintptr_t)out & 15) ||
        !conv_h16_eligible(ctx->use_h16, l2.k, l2.stride, l2.cin_pad16 / 2, l2.cout_pad, H, W, B, 0, 64))
        return 0;
    ConvParams p = conv_params(image, (const float*)(wts.f16 + l2.w16_off), wts.f32 + l2.b_off, out, B, H, W, H, W, l2.cin_pad16 / 2, 3, 64, 64, 64, 1, 1, 1);
    p.wpk1 = wts.f32 + l1.w_off; p.bias1 = wts.f32 + l1.b_off;
    p.im2col = 1; p.f16 = 1;
    const double px = (double)B * H * W;
    const double flops = 2.0 * 9 * (3.0 * 64 + 64.0 * 64) * px;
    const double bytes = px * 12 + 2.0 * (9 * 3 * 64 + 9 * 64 * 64) + 2.0 * px / 4 * 64;
    ProfScope ps(ctx, l2.name, "conv_h16_fused_c1_1+c1_2_pool", flops, bytes);
    ++ctx->conv_h16_launches;
    p.first_form = ctx->fuse12 == 2 ? 1 : ctx->fuse12 == 3 ? 2 : 0;
    const int form = conv_h16_fused12_launch(p, ctx->stream);
    if (form < 0) HP3D_FAIL(ctx, HP3D_ERR_UNSUPPORTED, "conv_h16 fused launch failed for %s", l2.name.c_str());
    if (form == 2) ++ctx->conv_h16_first_resident_launches;
    *oh = H / 2; *ow = W / 2;
    return 1;
}

// VGG-style trunk shared by HandSegNet and PoseNet2D: conv1_1 (im2col) ... through block 4's first
// `n4` layers.  Returns the activation pointer / size after the trunk.
int run_trunk(hp3d_ctx* ctx, const char* scope, const float* image, int B, int H, int W, int n4, float** act, int* h,
              int* w, bool input_hot) {
    ctx->trunk_input_hot = input_hot;
    char nm[64];
    float* a = ctx->bufA;
    float* b = ctx->bufB;
    const int f16 = ctx->prec;        // activations below are halves when set (same buffers, half the bytes)
    int ch = 64, ih = H, iw = W;
    snprintf(nm, sizeof nm, "%s/conv1_1", scope);
    char nm2[64];
    snprintf(nm2, sizeof nm2, "%s/conv1_2", scope);
    int first = 1, fh = 0, fw = 0;
    const int fused = f16 ? run_fused12(ctx, ConvW{ctx->blob, ctx->blob16, nullptr}, f16, CL(ctx, nm), CL(ctx, nm2), image, B, ih, iw, a, &fh, &fw) : 0;
    if (fused < 0) return fused;
    if (fused) { first = 2; ih = fh; iw = fw; }
    else CHK(run_conv(ctx, CL(ctx, nm), image, 3, B, ih, iw, a, 64, 0, nullptr, nullptr, f16));   // im2col fused in the loader
    const int nl[4] = {2, 2, 4, n4}, chs[4] = {64, 128, 256, 512};
    for (int blk = 0; blk < 4; ++blk) {
        for (int i = (blk == 0 ? first : 0); i < nl[blk]; ++i) {
            snprintf(nm, sizeof nm, "%s/conv%d_%d", scope, blk + 1, i + 1);
            const int pool = (blk < 3 && i == nl[blk] - 1) ? 1 : 0;
            int oh, ow;
            CHK(run_conv(ctx, CL(ctx, nm), a, ch, B, ih, iw, b, chs[blk], pool, &oh, &ow, f16));
            std::swap(a, b);
            ch = chs[blk]; ih = oh; iw = ow;
        }
    }
    *act = a; *h = ih; *w = iw;
    return 0;
}

// HandSegNet (nets/ColorHandPose3DNetwork.py:131-168) -> d_segsmall [B,H/8,W/8,32] (channels 0,1 real)
int run_handsegnet(hp3d_ctx* ctx, const float* image, int B, int H, int W, bool image_hot = false) {
    float* a; int h, w;
    CHK(run_trunk(ctx, "HandSegNet", image, B, H, W, 4, &a, &h, &w, image_hot));
    float* b = (a == ctx->bufA) ? ctx->bufB : ctx->bufA;
    const int f16 = ctx->prec;
    CHK(run_conv(ctx, CL(ctx, "HandSegNet/conv5_1"), a, 512, B, h, w, b, 512, 0, nullptr, nullptr, f16));
    CHK(run_conv(ctx, CL(ctx, "HandSegNet/conv5_2"), b, 512, B, h, w, a, 128, 0, nullptr, nullptr, f16));
    // conv6_1 (1x1, 128 -> 512) + conv6_2 (1x1, 512 -> 2): one launch where conv_pw2.hip takes the pair (the 512-channel map stays in LDS)
    const int fused = run_pw2(ctx, CL(ctx, "HandSegNet/conv6_1"), CL(ctx, "HandSegNet/conv6_2"), a, 128, B, h, w, ctx->d_segsmall, 32);
    if (fused < 0) return fused;
    if (fused) return 0;
    CHK(run_conv(ctx, CL(ctx, "HandSegNet/conv6_1"), a, 128, B, h, w, b, 512, 0, nullptr, nullptr, f16));
    // the 2-class head always leaves float32 logits for the softmax / mask stage
    CHK(run_conv(ctx, CL(ctx, "HandSegNet/conv6_2"), b, 512, B, h, w, ctx->d_segsmall, 32, 0, nullptr, nullptr, f16, 1));
    return 0;
}

// PoseNet2D (nets/ColorHandPose3DNetwork.py:170-219) -> d_sm[0..2] [B,h/8,w/8,32] (21 real channels)
int run_posenet(hp3d_ctx* ctx, const float* crop, int B, int H, int W, bool crop_hot = false) {
    float* a; int h, w;
    CHK(run_trunk(ctx, "PoseNet2D", crop, B, H, W, 2, &a, &h, &w, crop_hot));
    CHK(ensure_pose_bufs(ctx, B, h, w));
    const int f16 = ctx->prec;
    // concat([scoremap, encoding]) buffer: f32 [B,h,w,160] or f16 [B,h,w,192] (64-half chunks); channel 0..127 =
    // encoding, 128..148 = score map, rest zero (the f16 pad 160..191 is zeroed when the buffer is allocated)
    const int ccs = f16 ? 192 : 160;
    float* cat = f16 ? (float*)ctx->d_concat16 : ctx->d_concat;
    float* b = (a == ctx->bufA) ? ctx->bufB : ctx->bufA;
    CHK(run_conv(ctx, CL(ctx, "PoseNet2D/conv4_3"), a, 512, B, h, w, b, 256, 0, nullptr, nullptr, f16));
    CHK(run_conv(ctx, CL(ctx, "PoseNet2D/conv4_4"), b, 256, B, h, w, a, 256, 0, nullptr, nullptr, f16));
    CHK(run_conv(ctx, CL(ctx, "PoseNet2D/conv4_5"), a, 256, B, h, w, b, 256, 0, nullptr, nullptr, f16));
    CHK(run_conv(ctx, CL(ctx, "PoseNet2D/conv4_6"), b, 256, B, h, w, a, 256, 0, nullptr, nullptr, f16));
    CHK(run_conv(ctx, CL(ctx, "PoseNet2D/conv4_7"), a, 256, B, h, w, cat, ccs, 0, nullptr, nullptr, f16));
    // score-map heads always store float32 [.,32] (they feed the lifting nets, the up-sampler and the caller)
    {
        const int fused = f16 ? 0 : run_pw2(ctx, CL(ctx, "PoseNet2D/conv5_1"), CL(ctx, "PoseNet2D/conv5_2"), cat, ccs, B, h, w, ctx->d_sm[0], 32);
        if (fused < 0) return fused;
        if (!fused) {
            CHK(run_conv(ctx, CL(ctx, "PoseNet2D/conv5_1"), cat, ccs, B, h, w, a, 512, 0, nullptr, nullptr, f16));
            CHK(run_conv(ctx, CL(ctx, "PoseNet2D/conv5_2"), a, 512, B, h, w, ctx->d_sm[0], 32, 0, nullptr, nullptr, f16, 1));
        }
    }
    char nm[64];
    const int npix = B * h * w;
    for (int p = 0; p < 2; ++p) {
        // x = concat([scoremap, encoding]) : scoremap (21 real + 11 zero) -> channels 128..159
        if (f16) cvt_channels_f16_launch(ctx->d_sm[p], npix, 32, 32, ctx->d_concat16 + 128, 192, ctx->stream);
        else copy_channels_launch(ctx->d_sm[p], npix, 32, 32, ctx->d_concat + 128, 160, ctx->stream);
        const float* x = cat;
        int xcs = ccs;
        float* o = a;
        for (int r = 1; r <= 5; ++r) {
            snprintf(nm, sizeof nm, "PoseNet2D/conv%d_%d", p + 6, r);
            CHK(run_conv(ctx, CL(ctx, nm), x, xcs, B, h, w, o, 128, 0, nullptr, nullptr, f16));
            x = o; xcs = 128;
            o = (o == a) ? b : a;
        }
        char nm7[64];
        snprintf(nm, sizeof nm, "PoseNet2D/conv%d_6", p + 6);
        snprintf(nm7, sizeof nm7, "PoseNet2D/conv%d_7", p + 6);
        const int fused = f16 ? 0 : run_pw2(ctx, CL(ctx, nm), CL(ctx, nm7), x, 128, B, h, w, ctx->d_sm[p + 1], 32);
        if (fused < 0) return fused;
        if (!fused) {
            CHK(run_conv(ctx, CL(ctx, nm), x, 128, B, h, w, o, 128, 0, nullptr, nullptr, f16));
            CHK(run_conv(ctx, CL(ctx, nm7), o, 128, B, h, w, ctx->d_sm[p + 1], 32, 0, nullptr, nullptr, f16, 1));
        }
    }
    return 0;
}

// x2 != nullptr: the layer's last two inputs are the hand-side one-hot (concat(flatten, hand_side), :262-263 / :297-298, read in place)
int run_fc(hp3d_ctx* ctx, const FcL& l, const float* x, int B, int x_stride, float* out, int out_stride, const float* x2 = nullptr) {
    ProfScope ps(ctx, l.name, "fc", 2.0 * l.cin * l.cout * B, 4.0 * ((double)l.cin * l.cout + (double)B * (l.cin + l.cout)));
    fc_launch(x, B, l.cin, x_stride, ctx->blob + l.w_off, ctx->blob + l.b_off, l.cout, l.relu, out, out_stride,
              ctx->d_fcpart, ctx->stream, x2, l.cin - 2);
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

// the three FC layers of a tower as two launches (round 6): the K slices of the first, then its reduction + the two small layers (glue.hip: fc_tail_kernel)
int run_fc_tail(hp3d_ctx* ctx, const FcL& l0, const FcL& l1, const FcL& l2, const float* x, int B, int x_stride, const float* hs, float* out, int out_stride) {
    int ns;
    {
        ProfScope ps(ctx, l0.name, "fc_partial", 2.0 * l0.cin * l0.cout * B, 4.0 * ((double)l0.cin * l0.cout + (double)B * (l0.cin + l0.cout)));
        ns = fc_partial_launch(x, B, l0.cin, x_stride, ctx->blob + l0.w_off, l0.cout, ctx->d_fcpart, ctx->stream, hs, l0.cin - 2);
    }
    {
        ProfScope ps(ctx, l1.name + "+" + l2.name.substr(l2.name.find('/') + 1), "fc_tail", 2.0 * B * ((double)l1.cin * l1.cout + (double)l2.cin * l2.cout),
                     4.0 * ((double)l1.cin * l1.cout + (double)l2.cin * l2.cout + (double)ns * B * l0.cout));
        fc_tail_launch(ctx->d_fcpart, ns, B, l0.cout, ctx->blob + l0.b_off, l0.relu, ctx->blob + l1.w_off, ctx->blob + l1.b_off, l1.cout, l1.relu,
                       ctx->blob + l2.w_off, ctx->blob + l2.b_off, l2.cout, l2.relu, out, out_stride, ctx->stream);
    }
    ++ctx->fc_tail_launches;
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

// _inference_pose3d_can (nets/ColorHandPose3DNetwork.py:249-272; bottleneck: nets/PosePriorNetwork.py:115-116)
int run_poseprior_can(hp3d_ctx* ctx, const float* sm32 /*[B,32,32,32]*/, const float* hs, int B, int bottleneck,
                      float* can) {
    char nm[64];
    const float* x = sm32;
    int cs = 32, h = 32, w = 32;
    float* a = ctx->bufA;
    float* b = ctx->bufB;
    const int ch[3] = {32, 64, 128};
    for (int i = 0; i < 3; ++i) {
        snprintf(nm, sizeof nm, "PosePrior/conv_pose_%d_1", i);
        CHK(run_conv(ctx, CL(ctx, nm), x, cs, B, h, w, a, ch[i], 0, &h, &w));
        snprintf(nm, sizeof nm, "PosePrior/conv_pose_%d_2", i);
        CHK(run_conv(ctx, CL(ctx, nm), a, ch[i], B, h, w, b, ch[i], 0, &h, &w));
        x = b; cs = ch[i];   // next pair: b -> a -> b (no aliasing)
    }
    // x: [B,4,4,128] contiguous == NHWC flatten (h,w,c)
    CHK(run_fc(ctx, FL(ctx, "PosePrior/fc_rel0"), x, B, 2048, ctx->d_fc1, 512, hs));
    // (round 6: ViewpointNet's tail runs as one launch, fc_tail_kernel; here that form measured SLOWER -- the 512 x 512 layer is a 1 MB weight
    //  stream per workgroup (60 us), and with that layer kept on fc_partial the 512 -> 63 layer's K loop alone took 39 us: three plain FC layers stay)
    CHK(run_fc(ctx, FL(ctx, "PosePrior/fc_rel1"), ctx->d_fc1, B, 512, ctx->d_fc2, 512));
    if (bottleneck) {
        CHK(run_fc(ctx, FL(ctx, "PosePrior/fc_bottleneck"), ctx->d_fc2, B, 512, ctx->d_fc1, 32));
        CHK(run_fc(ctx, FL(ctx, "PosePrior/fc_xyz#bn"), ctx->d_fc1, B, 32, can, 63));
    } else {
        CHK(run_fc(ctx, FL(ctx, "PosePrior/fc_xyz"), ctx->d_fc2, B, 512, can, 63));
    }
    return 0;
}

// _rotation_estimation (nets/ColorHandPose3DNetwork.py:285-309) -> u [B,3]
int run_viewpoint(hp3d_ctx* ctx, const float* sm32, const float* hs, int B, float* u) {
    char nm[64];
    const float* x = sm32;
    int cs = 32, h = 32, w = 32;
    float* a = ctx->bufA;
    float* b = ctx->bufB;
    const int ch[3] = {64, 128, 256};
    for (int i = 0; i < 3; ++i) {
        snprintf(nm, sizeof nm, "ViewpointNet/conv_vp_%d_1", i);
        CHK(run_conv(ctx, CL(ctx, nm), x, cs, B, h, w, a, ch[i], 0, &h, &w));
        snprintf(nm, sizeof nm, "ViewpointNet/conv_vp_%d_2", i);
        CHK(run_conv(ctx, CL(ctx, nm), a, ch[i], B, h, w, b, ch[i], 0, &h, &w));
        x = b; cs = ch[i];   // next pair: b -> a -> b (no aliasing)
    }
    if (ctx->fc_tail && fc_tail_eligible(256, 128, 3)) {
        CHK(run_fc_tail(ctx, FL(ctx, "ViewpointNet/fc_vp0"), FL(ctx, "ViewpointNet/fc_vp1"), FL(ctx, "ViewpointNet/fc_vp_u"), x, B, 4096, hs, u, 3));
        return 0;
    }
    CHK(run_fc(ctx, FL(ctx, "ViewpointNet/fc_vp0"), x, B, 4096, ctx->d_fc1, 256, hs));
    CHK(run_fc(ctx, FL(ctx, "ViewpointNet/fc_vp1"), ctx->d_fc1, B, 256, ctx->d_fc2, 128));
    CHK(run_fc(ctx, FL(ctx, "ViewpointNet/fc_vp_u"), ctx->d_fc2, B, 128, u, 3));
    return 0;
}

// lift_fused.hip's grid barrier gives up after a bounded spin (a workgroup that is not resident would otherwise hang the GPU) and
// raises this word; every synchronisation point of the executor turns it into an error instead of handing out garbage.
int check_lift_error(hp3d_ctx* ctx) {
    if (ctx->h_lifterr && *(volatile unsigned*)ctx->h_lifterr) {
        *ctx->h_lifterr = 0;
        HP3D_FAIL(ctx, HP3D_ERR_HIP, "lift_fused: grid barrier timed out (a workgroup was not resident); the outputs of that call are invalid -- "
                                     "set option lift_fused=0 on a shared GPU");
    }
    if (ctx->kid) return check_lift_error(ctx->kid);
    return 0;
}

// _inference_pose3d (nets/ColorHandPose3DNetwork.py:221-247)
// The same two towers as ONE launch (lift_fused.hip): small batches, where 24 dependent launches of ~13 us are the cost
int run_lift_fused(hp3d_ctx* ctx, const float* sm32, const float* hs, int B, int bottleneck, int do_rot) {
    LiftFusedParams p;
    memset(&p, 0, sizeof p);
    p.sm = sm32; p.sm_cs = 32; p.hs = hs; p.B = B; p.towers = do_rot ? 3 : 1;
    char nm[64];
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 6; ++i) {
            snprintf(nm, sizeof nm, t == 0 ? "PosePrior/conv_pose_%d_%d" : "ViewpointNet/conv_vp_%d_%d", i / 2, i % 2 + 1);
            const ConvL& l = CL(ctx, nm);
            p.w[t * 6 + i] = ctx->blob + l.raw_off; p.b[t * 6 + i] = ctx->blob + l.b_off;
            p.cin[t * 6 + i] = l.cin4; p.cout[t * 6 + i] = l.cout;
        }
    const char* fcn[6] = {"PosePrior/fc_rel0", "PosePrior/fc_rel1", bottleneck ? "PosePrior/fc_xyz#bn" : "PosePrior/fc_xyz",
                          "ViewpointNet/fc_vp0", "ViewpointNet/fc_vp1", "ViewpointNet/fc_vp_u"};
    for (int f = 0; f < 6; ++f) {
        const FcL& l = FL(ctx, fcn[f]);
        p.fw[f] = ctx->blob + l.w_off; p.fb[f] = ctx->blob + l.b_off; p.fc_in[f] = l.cin; p.fc_out[f] = l.cout;
    }
    if (bottleneck) {
        const FcL& l = FL(ctx, "PosePrior/fc_bottleneck");
        p.bn_w = ctx->blob + l.w_off; p.bn_b = ctx->blob + l.b_off;
        p.fc_in[2] = 512;             // the last stage reads fc_rel1's 512 outputs; the 30-wide layer sits inside it
    }
    const size_t act = (size_t)B * 32 * 32 * 64;
    for (int t = 0; t < 2; ++t)
        for (int q = 0; q < 2; ++q) p.act[t][q] = ctx->bufA + (size_t)(t * 2 + q) * act;
    float* fp = ctx->d_fcpart;
    p.fcp[0][0] = fp; fp += (size_t)9 * B * 512;
    p.fcp[0][1] = fp; fp += (size_t)2 * B * 512;
    p.fcp[1][0] = fp; fp += (size_t)17 * B * 256;
    p.fcp[1][1] = fp;
    p.out[0] = ctx->d_can; p.out[1] = ctx->d_u;
    if (!ctx->d_liftbar) CHK(dev_realloc(ctx, &ctx->d_liftbar, 4));
    p.bar = ctx->d_liftbar;
#ifndef HP3D_EMU
    if (!ctx->h_lifterr) {
        HIPCHK(ctx, hipHostMalloc((void**)&ctx->h_lifterr, sizeof(unsigned), hipHostMallocMapped));
        *ctx->h_lifterr = 0;
    }
    CHK(check_lift_error(ctx));            // an earlier launch of this context already failed: do not pile work on garbage
    HIPCHK(ctx, hipHostGetDevicePointer((void**)&p.err, ctx->h_lifterr, 0));
#endif
    ProfScope ps(ctx, "PosePrior+ViewpointNet", "lift_fused", 2.0 * B * (45.0e6 / 2 + 157.0e6 / 2 * (do_rot ? 1 : 0) + 2.7e6 / 2), 4.0 * 15.5e6);
    if (lift_fused_launch(p, ctx->stream)) HP3D_FAIL(ctx, HP3D_ERR_HIP, "lift_fused launch failed");
    ++ctx->lift_fused_launches;
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

int kid_sync_state(hp3d_ctx* ctx);

// The child context's share of an overlapped lifting stage: ViewpointNet's activations ([B,32,32,64] is the largest), its FC buffers
// and split-K partial sums.  (A later two-stream call grows the same arena through ensure_arena.)
int ensure_side_tower(hp3d_ctx* k, int B) {
    const size_t act = (size_t)B * 32 * 32 * 64;
    if (act > k->act_floats) {
        CHK(dev_realloc(k, &k->bufA, act));
        CHK(dev_realloc(k, &k->bufB, act));
        k->act_floats = act;
    }
    if (B > k->sideB) {
        CHK(dev_realloc(k, &k->d_fc1, (size_t)B * 512));
        CHK(dev_realloc(k, &k->d_fc2, (size_t)B * 512));
        CHK(dev_realloc(k, &k->d_fcpart, std::max((size_t)B * 17 * 512 + (size_t)B * 33 * 256, (size_t)B * 16 * 18 * 256)));
        k->sideB = B;
    }
    return 0;
}

// `beside` (may be null): work of the caller that depends on neither tower (the whole path's heat-map up-sampling and keypoint detection);
// it runs on this context's stream behind PosePrior -- i.e. beside ViewpointNet when the towers run on two streams -- and before the epilogue.
// `beside_side` (round 6, may be null): the part of that work that goes BEHIND ViewpointNet on the child stream instead when the towers run on two
// streams -- since ViewpointNet's tower got shorter (fc_tail, conv_s2_gemm: 0.206 -> 0.179 ms) the parent stream (PosePrior 0.15 + up-sampling 0.037 +
// keypoint detection 0.055) was the longer one; with the up-sampling on the child both are ~0.21 ms.  One stream: it simply runs after `beside`.
int run_pose3d(hp3d_ctx* ctx, const float* sm32, const float* hs, int B, int variant, const std::function<int(hipStream_t)>* beside = nullptr,
               const std::function<int(hipStream_t)>* beside_side = nullptr) {
    const int do_rot = (variant == HP3D_VARIANT_PROPOSED);
    const bool fused = !ctx->conv_naive && (ctx->use_lift_fused == 1 || (ctx->use_lift_fused < 0 && B <= 4)) &&
                       (size_t)4 * B * 32 * 32 * 64 <= ctx->act_floats;
    if (fused) {
        CHK(run_lift_fused(ctx, sm32, hs, B, variant == HP3D_VARIANT_BOTTLENECK, do_rot));
    } else {
        // The two towers share only their input (nets/ColorHandPose3DNetwork.py:231-235): 12 + 12 dependent launches of 13-25 us each that
        // leave most of the chip idle.  ViewpointNet runs on the child context's stream (own activations and partial sums, shared weights)
        // beside PosePrior on this one; the epilogue below waits for both.  Not while profiling per launch, replaying a graph, or when
        // this context is (or is busy with) the second stream of a two-stream call.
        const bool side = do_rot && ctx->lift_overlap && !ctx->profiling && !ctx->use_graph && !ctx->conv_naive && !ctx->shared_weights &&
                          !ctx->two_streams_live && kid_sync_state(ctx) == 0 && ensure_side_tower(ctx->kid, B) == 0;
        if (side) {
            hp3d_ctx* k = ctx->kid;
            KidFork fork;
            CHK(fork.fork(ctx));
            const int rc = run_viewpoint(k, sm32, hs, B, ctx->d_u);
            if (rc != 0) { set_error(ctx, k->err.c_str()); return rc; }
            if (beside_side && ctx->kp_up_side) { CHK((*beside_side)(k->stream)); beside_side = nullptr; }
            CHK(run_poseprior_can(ctx, sm32, hs, B, variant == HP3D_VARIANT_BOTTLENECK, ctx->d_can));
            if (beside) { CHK((*beside)(ctx->stream)); beside = nullptr; }
            ++ctx->lift_overlap_calls;
        } else {
            CHK(run_poseprior_can(ctx, sm32, hs, B, variant == HP3D_VARIANT_BOTTLENECK, ctx->d_can));
            if (do_rot) CHK(run_viewpoint(ctx, sm32, hs, B, ctx->d_u));
        }
    }
    if (beside) CHK((*beside)(ctx->stream));
    if (beside_side) CHK((*beside_side)(ctx->stream));
    if (variant == HP3D_VARIANT_LOCAL)     // bone_rel_trafo_inv (nets/PosePriorNetwork.py:70-75)
        bone_rel_inv_launch(ctx->d_can, B, ctx->d_coord, ctx->stream);
    else
        lift_epilogue_launch(ctx->d_u, ctx->d_can, hs, B, ctx->d_rot, ctx->d_coord, do_rot, ctx->stream);
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

int need_nets(hp3d_ctx* ctx, int mask) {
    if (!ctx->blob) HP3D_FAIL(ctx, HP3D_ERR_WEIGHTS, "weights not finalized (call hp3d_finalize_weights)");
    if ((ctx->nets & mask) != mask)
        HP3D_FAIL(ctx, HP3D_ERR_WEIGHTS, "required network weights not loaded (have mask %d, need %d)", ctx->nets, mask);
    return 0;
}

// The frame-size envelope: the largest per-image activation (conv1_1 / conv1_2: H x W x 64 floats) must stay below 2^31 bytes, the
// 32-bit offsets the convolution kernels address a chunk with (auto_micro_batch then cuts a call into chunks that keep it) -- up to
// 8388607 pixels: 2160x3840 is inside.
int check_img(hp3d_ctx* ctx, int B, int H, int W) {
    if (B < 1 || H < 16 || W < 16)
        HP3D_FAIL(ctx, HP3D_ERR_ARG, "bad shape B=%d H=%d W=%d (need B>=1, H,W >=16)", B, H, W);
    if ((long)H * W * 64 * 4 >= (1L << 31))
        HP3D_FAIL(ctx, HP3D_ERR_ARG, "image %dx%d too large: H*W*64*4 bytes (one image's largest activation) must stay below 2^31", H, W);
    if (ctx->mask_grow == 1 && !mask_grow_lds_fits(H, W))
        HP3D_FAIL(ctx, HP3D_ERR_ARG, "image %dx%d too large for the in-LDS mask growth", H, W);
    return 0;
}

int copy_in(hp3d_ctx* ctx, float* dst, const float* src, size_t n, bool dev) {
    HIPCHK(ctx, hipMemcpyAsync(dst, src, n * sizeof(float), dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                               ctx->stream));
    return 0;
}
int copy_out(hp3d_ctx* ctx, float* dst, const float* src, size_t n, bool dev) {
    if (!dst) return 0;
    HIPCHK(ctx, hipMemcpyAsync(dst, src, n * sizeof(float), dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                               ctx->stream));
    return 0;
}

// stages 2-8 of the full path on device-resident image/hand_side
// K > 0: the multi-hand form -- HandSegNet once, the soft-max also writes fg, up to K hands per image into slots
// b * K + j of d_center / d_scale / d_cropsize / d_seed / d_valid / d_area (/ d_mask), and B * K crops from the B frames
// mk (K > 0): the slots a multi-hand tracking step keeps; that step crops itself (do_crop = false)
int run_detect_and_crop(hp3d_ctx* ctx, const float* d_image, int B, int H, int W, int want_mask, bool image_hot = false, bool do_crop = true,
                        int K = 0, const MaskKeep& mk = MaskKeep()) {
    CHK(run_handsegnet(ctx, d_image, B, H, W, image_hot));
    MaskBuffers mb{ctx->d_keys, ctx->d_det, K > 0 ? ctx->d_fg : nullptr};
    {
        ProfScope ps(ctx, "seg_upsample_softmax", "seg_upsample_softmax", 0.0, 4.0 * B * H * W * 2 + (double)B * H * W);
        seg_upsample_softmax_launch(ctx->d_segsmall, B, H / 8, W / 8, 32, H, W, ctx->d_large, mb, ctx->stream);
    }
    if (K > 0) {
        {
            ProfScope ps(ctx, "mask_grow_multi", "mask_grow_multi", 0.0, (double)B * H * W * 5);
            const bool global = mask_grow_global(ctx, H, W);
            mask_grow_multi_launch(mb, B, H, W, K, ctx->hands_min_area, ctx->empty_fltmax, global ? ctx->d_mgscratch : nullptr,
                                   want_mask ? ctx->d_mask : nullptr, ctx->d_center, ctx->d_cropsize, ctx->d_scale, ctx->d_seed, ctx->d_valid,
                                   ctx->d_area, ctx->stream, mk);
            ++ctx->mask_grow_multi_launches;
            if (global) ++ctx->mask_grow_global_launches;
        }
        if (!do_crop) { HIPCHK(ctx, hipGetLastError()); return 0; }
        ProfScope ps(ctx, "crop_and_resize", "crop_and_resize", 0.0, 4.0 * B * (H * W * 3 + K * 256 * 256 * 3));
        crop_and_resize_launch(d_image, B * K, H, W, 3, ctx->d_center, ctx->d_scale, 256, ctx->d_crop, ctx->stream, K);
        HIPCHK(ctx, hipGetLastError());
        return 0;
    }
    {
        ProfScope ps(ctx, "mask_grow", "mask_grow", 0.0, (double)B * H * W);
        if (mask_grow_global(ctx, H, W)) {
            mask_grow_global_launch(mb, B, H, W, ctx->empty_fltmax, ctx->d_mgscratch, want_mask ? ctx->d_mask : nullptr, ctx->d_center,
                                    ctx->d_cropsize, ctx->d_scale, ctx->d_seed, ctx->stream);
            ++ctx->mask_grow_global_launches;
        } else {
            mask_grow_launch(mb, B, H, W, ctx->empty_fltmax, want_mask ? ctx->d_mask : nullptr, ctx->d_center,
                             ctx->d_cropsize, ctx->d_scale, ctx->d_seed, ctx->stream);
        }
    }
    if (do_crop) {          // (a tracking step chooses its boxes first: track_step_impl)
        ProfScope ps(ctx, "crop_and_resize", "crop_and_resize", 0.0, 4.0 * B * (H * W * 3 + 256 * 256 * 3));
        crop_and_resize_launch(d_image, B, H, W, 3, ctx->d_center, ctx->d_scale, 256, ctx->d_crop, ctx->stream);
    }
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

// detect_keypoints + trafo_coords (utils/general.py:331-357; run.py:72-73, eval2d.py:93-94) on the 32 x 32 maps of the
// last PoseNet2D run: no 256 x 256 x 21 heat-map has to exist, let alone travel to the host
int run_kp_detect(hp3d_ctx* ctx, int B, int32_t* kp_crop, double* kp_image, bool dev, const float* scale = nullptr, const float* center = nullptr) {
    ProfScope ps(ctx, "kp_detect", "kp_detect", 0.0, 4.0 * B * 32 * 32 * 21);
    kp_detect_launch(ctx->d_sm[2], B, 32, 32, 21, 32, 256, 256, scale ? scale : ctx->d_scale, center ? center : ctx->d_center,
                     dev && kp_crop ? kp_crop : ctx->d_kpcrop, dev && kp_image ? kp_image : ctx->d_kpimg, ctx->stream);
    HIPCHK(ctx, hipGetLastError());
    if (!dev) {
        if (kp_crop) HIPCHK(ctx, hipMemcpyAsync(kp_crop, ctx->d_kpcrop, sizeof(int32_t) * (size_t)B * 42, hipMemcpyDeviceToHost, ctx->stream));
        if (kp_image) HIPCHK(ctx, hipMemcpyAsync(kp_image, ctx->d_kpimg, sizeof(double) * (size_t)B * 42, hipMemcpyDeviceToHost, ctx->stream));
    }
    return 0;
}

int infer_full_impl(hp3d_ctx* ctx, int B, int H, int W, const float* image, const float* hand_side,
                    float* hand_scoremap, float* image_crop, float* scale_crop, float* center, float* kp_scoremap,
                    float* coord3d, float* hand_mask, bool dev, const unsigned char* image_u8 = nullptr, int Hin = 0,
                    int Win = 0, int32_t* kp_crop = nullptr, double* kp_image = nullptr, bool no_sync = false) {
    if (!ctx) return HP3D_ERR_ARG;
    if ((!image && !image_u8) || !hand_side) HP3D_FAIL(ctx, HP3D_ERR_ARG, "image / hand_side is NULL");
    CHK(check_img(ctx, B, H, W));
    CHK(need_nets(ctx, NET_SEG | NET_POSE | NET_PRIOR | NET_VP));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    CHK(ensure_arena(ctx, B, H, W));
    if (ctx->profiling != 2) prof_reset(ctx);   // mode 2 accumulates across calls
    const float* d_img = image;
    const float* d_hs = hand_side;
    if (image_u8) {          // uint8 frame in, x/255-0.5 + resize to the net size on device
        if (Hin < 2 || Win < 2) HP3D_FAIL(ctx, HP3D_ERR_ARG, "bad uint8 frame size %dx%d", Hin, Win);
        const size_t nb = (size_t)B * Hin * Win * 3;
        if (nb > ctx->u8_bytes) { CHK(dev_realloc(ctx, &ctx->d_u8, nb)); ctx->u8_bytes = nb; }
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_u8, image_u8, nb, hipMemcpyHostToDevice, ctx->stream));
        preprocess_u8_launch(ctx->d_u8, B, Hin, Win, H, W, ctx->d_image, ctx->stream);
        CHK(copy_in(ctx, ctx->d_hs, hand_side, (size_t)B * 2, false));
        d_img = ctx->d_image; d_hs = ctx->d_hs;
    } else if (!dev) {
        CHK(copy_in(ctx, ctx->d_image, image, (size_t)B * H * W * 3, false));
        CHK(copy_in(ctx, ctx->d_hs, hand_side, (size_t)B * 2, false));
        d_img = ctx->d_image; d_hs = ctx->d_hs;
    }
    CHK(run_detect_and_crop(ctx, d_img, B, H, W, hand_mask != nullptr, image_u8 != nullptr));     // (the uint8 front end has just written the image)
    CHK(run_posenet(ctx, ctx->d_crop, B, 256, 256, true));
    // (the heat-map up-sampling and the keypoint detection read PoseNet2D's last score map like the lifting towers do and depend on neither:
    //  they run beside ViewpointNet when the towers take two streams, option "lift_overlap")
    const std::function<int(hipStream_t)> kp_up = [&](hipStream_t st) -> int {
        if (kp_scoremap) {
            ProfScope ps(ctx, "kp_upsample", "resize_bilinear", 0.0, 4.0 * B * (32 * 32 * 21 + 256 * 256 * 21));
            resize_bilinear_launch(ctx->d_sm[2], B, 32, 32, 21, 32, 256, 256, dev ? kp_scoremap : ctx->d_kpmap, st);
        }
        return 0;
    };
    const std::function<int(hipStream_t)> kp_work = [&](hipStream_t) -> int {
        if (kp_crop || kp_image) CHK(run_kp_detect(ctx, B, kp_crop, kp_image, dev));
        return 0;
    };
    CHK(run_pose3d(ctx, ctx->d_sm[2], d_hs, B, HP3D_VARIANT_PROPOSED, &kp_work, &kp_up));
    CHK(copy_out(ctx, hand_scoremap, ctx->d_large, (size_t)B * H * W * 2, dev));
    CHK(copy_out(ctx, image_crop, ctx->d_crop, (size_t)B * 256 * 256 * 3, dev));
    CHK(copy_out(ctx, scale_crop, ctx->d_scale, (size_t)B, dev));
    CHK(copy_out(ctx, center, ctx->d_center, (size_t)B * 2, dev));
    if (!dev) CHK(copy_out(ctx, kp_scoremap, ctx->d_kpmap, (size_t)B * 256 * 256 * 21, false));
    CHK(copy_out(ctx, coord3d, ctx->d_coord, (size_t)B * 63, dev));
    CHK(copy_out(ctx, hand_mask, ctx->d_mask, (size_t)B * H * W, dev));
    if (!dev && !no_sync) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// Large batches run as consecutive chunks of micro_batch images: per-layer activations of one chunk (<= 0.84 GB at
// 320x320) stay closer to the caches and every tensor stays inside the 32-bit offsets of the Winograd kernel.  Measured:
// f32 320x320 B=32 1452 img/s, B=128 unsplit 1355, split 4 x 32 1460; f16 480x640 B=128 unsplit 2316, split 2072 --
// hence auto = at most 32 for float32, no split for the half-precision mode.  The float32 limit also follows the
// resolution: the largest activation of the path (conv1_1 / conv1_2: H x W x 64 floats per image) must stay below 2^31
// bytes per chunk or those layers fall off the Winograd kernel (480x640: 27 images), and the chunks are balanced
// (B = 32 at 480x640 -> 16 + 16, not 27 + 5) so that no chunk under-fills the persistent grids.
int auto_micro_batch(const hp3d_ctx* ctx, int B, int H, int W) {
    if (ctx->micro_batch >= 0) return ctx->micro_batch;
    if (ctx->prec) return 0;
    const long per_img = (long)H * W * 64 * 4;
    int lim = (int)std::min<long>(32, ((1L << 31) - 1) / std::max<long>(per_img, 1));
    if (lim < 1) lim = 1;
    if (B <= lim) return lim;
    // 32 images fill every persistent grid of the path at the reference's sizes (exactly 256 conv_wino7 items, whole rounds of conv_wino4
    // items on most layers): chunks of 32 and a remainder beat balanced chunks there (round 5, 320x320: B = 48 as 24 + 24: 20.16 ms;
    // as 32 + 16: 11.99 + 6.70).  Where the 32-bit offsets allow fewer than 32 images per chunk the chunks stay balanced.
    // (ADVICE r5 asked whether a small remainder -- B = 33 ... 40 -- should rather be balanced: measured in round 6, B = 40 at 320x320 as 32 + 8:
    //  16.09 ms, as 20 + 20: 16.65 ms.  The full chunk keeps its rate; what helps such batches is the second stream, see infer_full_streams.)
    if (lim == 32) return 32;
    const int chunks = (B + lim - 1) / lim;
    return (B + chunks - 1) / chunks;
}

int infer_full_chunked1(hp3d_ctx* ctx, int B, int H, int W, const float* image, const float* hand_side,
                       float* hand_scoremap, float* image_crop, float* scale_crop, float* center, float* kp_scoremap,
                       float* coord3d, float* hand_mask, bool dev, const unsigned char* image_u8 = nullptr, int Hin = 0,
                       int Win = 0, int32_t* kp_crop = nullptr, double* kp_image = nullptr, bool no_sync = false) {
    if (!ctx) return HP3D_ERR_ARG;
    const int mb = auto_micro_batch(ctx, B, H, W);
    if (mb <= 0 || B <= mb)
        return infer_full_impl(ctx, B, H, W, image, hand_side, hand_scoremap, image_crop, scale_crop, center, kp_scoremap,
                               coord3d, hand_mask, dev, image_u8, Hin, Win, kp_crop, kp_image, no_sync);
    CHK(check_img(ctx, B, H, W));
    if (!hand_side) HP3D_FAIL(ctx, HP3D_ERR_ARG, "image / hand_side is NULL");
    const int saved_prof = ctx->profiling;
    int rc = 0;
    for (int b0 = 0; b0 < B && rc == 0; b0 += mb) {
        const int nb = std::min(mb, B - b0);
        auto off = [&](float* p, size_t per) { return p ? p + (size_t)b0 * per : nullptr; };
        if (b0 > 0 && saved_prof == 1) ctx->profiling = 2;          // one call = one profile: keep the earlier chunks
        rc = infer_full_impl(ctx, nb, H, W, image ? image + (size_t)b0 * H * W * 3 : nullptr, hand_side + (size_t)b0 * 2,
                             off(hand_scoremap, (size_t)H * W * 2), off(image_crop, 256 * 256 * 3), off(scale_crop, 1),
                             off(center, 2), off(kp_scoremap, 256 * 256 * 21), off(coord3d, 63), off(hand_mask, (size_t)H * W),
                             dev, image_u8 ? image_u8 + (size_t)b0 * Hin * Win * 3 : nullptr, Hin, Win,
                             kp_crop ? kp_crop + (size_t)b0 * 42 : nullptr, kp_image ? kp_image + (size_t)b0 * 42 : nullptr, no_sync);
    }
    ctx->profiling = saved_prof;
    return rc;
}

// Two HIP streams per GPU: the batch is cut in two halves that run the whole path concurrently, each on its own stream and
// arena (the second one owned by a child context that shares the weight blob).  Every image is independent, and the
// persistent Winograd kernels leave CUs idle in their last round of work items (1600 items on 256 CUs = 6.25 rounds) and
// between dependent launches: the other half's kernels fill exactly those holes.  Measured (profiles/r02_tuning_notes.md):
// float32 B=32 320x320 1558 -> 1615 img/s, 240x320 +1.8 %, 480x640 +6.9 %, B=16 +4.5 %, B=64 +6.4 %, f16 trunks +2.1 %; four
// streams of 8 images lose 8 % (too few items per launch); round 3's "auto" was 2 streams from 16 images per call; round 4: see `ns` below.
// Per-launch profiling and hipGraph replay keep one stream.  A half-batch may take another kernel plan than the whole
// batch would (small-batch Winograd split-K): results equal the one-stream run to rounding, discrete decisions included.
int kid_sync_state(hp3d_ctx* ctx) {
#ifdef HP3D_EMU
    return -1;
#else
    if (!ctx->kid) {
        hp3d_ctx* k = new hp3d_ctx();
        k->device = ctx->device;
        if (hipStreamCreateWithFlags(&k->stream, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            delete k;
            return -1;
        }
        k->shared_weights = true;
        ctx->kid = k;
    }
    hp3d_ctx* k = ctx->kid;
    k->blob = ctx->blob; k->blob16 = ctx->blob16; k->nets = ctx->nets; k->prec = ctx->prec;
    static_cast<Options&>(*k) = *ctx;
    k->nstreams = 1; k->profiling = 0; k->use_graph = 0;
    return 0;
#endif
}

int infer_full_chunked(hp3d_ctx* ctx, int B, int H, int W, const float* image, const float* hand_side,
                       float* hand_scoremap, float* image_crop, float* scale_crop, float* center, float* kp_scoremap,
                       float* coord3d, float* hand_mask, bool dev, const unsigned char* image_u8 = nullptr, int Hin = 0,
                       int Win = 0, int32_t* kp_crop = nullptr, double* kp_image = nullptr) {
    if (!ctx) return HP3D_ERR_ARG;
    // "auto": two streams when each half still fills the persistent grids -- from 2.4 M input pixels per half (3 M until round 6).  Round 4 (tail pieces took the
    // last-round quantisation out of the one-stream run; same box, float32, images/s one / two streams): B=32 320x320 2190 / 2115,
    // B=16 1975 / 1787, B=8 1666 / 1372, B=32 240x320 2454 / 2408 -- one stream; B=64 320x320 (two chunks of 32) 2195 / 2292, B=32 480x640
    // 989 / 1051, f16 B=128 480x640 3234 / 3321 -- two (profiles/r04_tuning_notes.md).
    // Round 6: also between one and two full chunks (32 < B < 64 in float32 mode), where one stream runs a full chunk and then a latency-bound
    // remainder: B = 40 at 320x320 2487 (32 + 8) -> 2616 images/s, B = 48 2591 -> 2622, 240x320 B = 48 2945 -> 3012 (profiles/r06_batch_sweep.txt).
    // (From 40 images: B = 36 as 18 + 18 on two streams 2151, as 32 beside 4 2466, on one stream ~2430 -- halves below 20 images are too small.
    //  A full chunk BESIDE the remainder instead of two halves loses from B = 40 on: 2502 / 2587 against 2609 / 2617 at B = 40 / 48.)
    const bool between = !ctx->prec && ctx->micro_batch < 0 && B >= 40 && B < 64 && (long)H * W <= 320L * 320L;
    const int ns = ctx->nstreams >= 0 ? ctx->nstreams : (((long)(B / 2) * H * W >= 2400000L || between) ? 2 : 1);        // (2.4 M: B = 64 at 240x320 3048 -> 3132)
    if (ns < 2 || B < 2 || ctx->profiling || ctx->use_graph || ctx->conv_naive || ctx->shared_weights || !hand_side ||
        (!image && !image_u8) || kid_sync_state(ctx) != 0)
        return infer_full_chunked1(ctx, B, H, W, image, hand_side, hand_scoremap, image_crop, scale_crop, center, kp_scoremap,
                                   coord3d, hand_mask, dev, image_u8, Hin, Win, kp_crop, kp_image);
    hp3d_ctx* k = ctx->kid;
    const int b0 = (B + 1) / 2, b1 = B - b0;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    KidFork fork;
    CHK(fork.fork(ctx, true));
    auto off = [&](float* p, size_t per) { return p ? p + (size_t)b0 * per : nullptr; };
    // (host buffers: the child's pageable device->host copies block the host, so the two halves overlap on the `_dev`
    //  entry points only -- the ones bench.py and dist.py use)
    int rc = infer_full_chunked1(k, b1, H, W, image ? image + (size_t)b0 * H * W * 3 : nullptr, hand_side + (size_t)b0 * 2,
                                 off(hand_scoremap, (size_t)H * W * 2), off(image_crop, 256 * 256 * 3), off(scale_crop, 1),
                                 off(center, 2), off(kp_scoremap, 256 * 256 * 21), off(coord3d, 63), off(hand_mask, (size_t)H * W),
                                 dev, image_u8 ? image_u8 + (size_t)b0 * Hin * Win * 3 : nullptr, Hin, Win,
                                 kp_crop ? kp_crop + (size_t)b0 * 42 : nullptr, kp_image ? kp_image + (size_t)b0 * 42 : nullptr, true);
    if (rc != 0) { set_error(ctx, k->err.c_str()); }
    const int rc0 = rc != 0 ? rc : infer_full_chunked1(ctx, b0, H, W, image, hand_side, hand_scoremap, image_crop, scale_crop, center,
                                                       kp_scoremap, coord3d, hand_mask, dev, image_u8, Hin, Win, kp_crop, kp_image, true);
    if (rc0 != 0) return rc0;
    // (the parent's stream continues only after the child's half is done: the join; host buffers: wait for both here)
    if (!dev) {
        HIPCHK(ctx, hipStreamSynchronize(k->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    return 0;
}

int posenet_impl(hp3d_ctx* ctx, int B, int H, int W, const float* image_crop, float* s0, float* s1, float* s2, bool dev) {
    if (!ctx) return HP3D_ERR_ARG;
    if (!image_crop) HP3D_FAIL(ctx, HP3D_ERR_ARG, "image_crop is NULL");
    CHK(check_img(ctx, B, H, W));
    CHK(need_nets(ctx, NET_POSE));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    CHK(ensure_arena(ctx, B, H, W));
    if (ctx->profiling != 2) prof_reset(ctx);   // mode 2 accumulates across calls
    const float* d_img = image_crop;
    if (!dev) {
        CHK(copy_in(ctx, ctx->d_image, image_crop, (size_t)B * H * W * 3, false));
        d_img = ctx->d_image;
    }
    CHK(run_posenet(ctx, d_img, B, H, W));
    const int hs = H / 8, ws = W / 8, npix = B * hs * ws;
    float* outs[3] = {s0, s1, s2};
    for (int i = 0; i < 3; ++i) {
        if (!outs[i]) continue;
        float* dst = dev ? outs[i] : ctx->bufA;   // compact [npix,21] staging
        copy_channels_launch(ctx->d_sm[i], npix, 21, 32, dst, 21, ctx->stream);
        if (!dev) {
            CHK(copy_out(ctx, outs[i], ctx->bufA, (size_t)npix * 21, false));
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        }
    }
    HIPCHK(ctx, hipGetLastError());
    if (!dev) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// scratch helpers for the per-op entry points (host in -> device -> host out)
struct Scratch {
    hp3d_ctx* ctx;
    std::vector<void*> ptrs;
    explicit Scratch(hp3d_ctx* c) : ctx(c) {}
    ~Scratch() {
        for (void* p : ptrs) hipFree(p);
    }
    template <typename T>
    T* alloc(size_t n) {
        void* p = nullptr;
        if (hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)) != hipSuccess) return nullptr;
        ptrs.push_back(p);
        return (T*)p;
    }
    template <typename T>
    T* upload(const T* h, size_t n) {
        T* d = alloc<T>(n);
        if (d && hipMemcpyAsync(d, h, n * sizeof(T), hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return nullptr;
        return d;
    }
};
#define NN(ctx, p)                                                         \
    do {                                                                   \
        if (!(p)) HP3D_FAIL(ctx, HP3D_ERR_NOMEM, "scratch allocation/upload failed: %s", #p); \
    } while (0)

int finish_op(hp3d_ctx* ctx) {
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return check_lift_error(ctx);
}

// ---- tracking ---------------------------------------------------------------------------------------
// Device state for B images; grown on the first step / seed of a larger batch, never inside a steady-state step.
int ensure_track(hp3d_ctx* ctx, int B) {
    TrackState& T = ctx->track;
    if (B <= T.cap) return 0;
    CHK(T.h_lost.wait(ctx));
    for (int i = 0; i < 2; ++i) {
        CHK(dev_realloc(ctx, &T.center[i], (size_t)B * 2));
        CHK(dev_realloc(ctx, &T.scale[i], (size_t)B));
    }
    CHK(dev_realloc(ctx, &T.conf, (size_t)B));
    CHK(dev_realloc(ctx, &T.lost, (size_t)B));
    CHK(dev_realloc(ctx, &T.detected, (size_t)B));
    CHK(dev_realloc(ctx, &T.pidx, (size_t)B));
    CHK(dev_realloc(ctx, &T.ppos, (size_t)B));
    CHK(T.h_lost.resize(ctx, (size_t)B, "tracking state"));
    T.cap = B;
    T.valid = false;
    return 0;
}

void track_free(hp3d_ctx* ctx) {
    TrackState& T = ctx->track;
    for (int i = 0; i < 2; ++i) {
        if (T.center[i]) hipFree(T.center[i]);
        if (T.scale[i]) hipFree(T.scale[i]);
    }
    if (T.conf) hipFree(T.conf);
    if (T.lost) hipFree(T.lost);
    if (T.detected) hipFree(T.detected);
    if (T.pidx) hipFree(T.pidx);
    if (T.ppos) hipFree(T.ppos);
    T.h_lost.free();
    T = TrackState();
}

// Option "detect_scale" = f > 1: a detect step of either tracker finds the hand on the [Hd, Wd] = [ceil(H / f),
// ceil(W / f)] area mean of the frame -- HandSegNet, the soft-max and the mask growth run there exactly as they run on a frame of that
// size -- maps the boxes to frame coordinates and crops from the frame itself.  The arena and the chunking follow (Hd, Wd); a host
// float32 frame is staged in a buffer of its own (d_image holds the detection frame).  f = 1: (Hd, Wd) = (H, W), nothing changes.
int detect_frame(hp3d_ctx* ctx, int H, int W, int* Hd, int* Wd) {
    const int f = ctx->detect_scale;
    *Hd = (H + f - 1) / f; *Wd = (W + f - 1) / f;
    if (f > 1 && (*Hd < 16 || *Wd < 16))
        HP3D_FAIL(ctx, HP3D_ERR_ARG, "detect_scale=%d: the detection frame of a %dx%d frame is %dx%d (need >= 16x16)", f, H, W, *Hd, *Wd);
    return 0;
}
int ensure_stage(hp3d_ctx* ctx, size_t floats) {
    if (floats > ctx->stage_floats) {
        CHK(dev_realloc(ctx, &ctx->d_stage, floats));
        ctx->stage_floats = floats;
    }
    return 0;
}
// ---- NV12 frames (layout and colour rule: include/hp3d.h) ------------------------------------------------------------
// What the caller handed over: frame 0's planes (host or device pointers), the row pitch, the frame stride.
struct Nv12Arg {
    const unsigned char* y;
    const unsigned char* uv;
    int pitch;
    long long frame_stride;
};
// every refusal comes before anything is enqueued
int check_nv12(hp3d_ctx* ctx, int B, int H, int W, const Nv12Arg& a) {
    if (!a.y) HP3D_FAIL(ctx, HP3D_ERR_ARG, "nv12: y (the luma plane) is NULL");
    if (!a.uv) HP3D_FAIL(ctx, HP3D_ERR_ARG, "nv12: uv (the chroma plane) is NULL");
    if (B < 1 || H < 16 || W < 16) HP3D_FAIL(ctx, HP3D_ERR_ARG, "bad shape B=%d H=%d W=%d (need B>=1, H,W >=16)", B, H, W);
    if ((H | W) & 1) HP3D_FAIL(ctx, HP3D_ERR_ARG, "nv12: H=%d and W=%d must be even (a chroma sample covers 2 x 2 pixels)", H, W);
    if (a.pitch < W) HP3D_FAIL(ctx, HP3D_ERR_ARG, "nv12: pitch=%d is below W=%d", a.pitch, W);
    if (B > 1 && a.frame_stride < (long long)a.pitch * (H - 1) + W)
        HP3D_FAIL(ctx, HP3D_ERR_ARG, "nv12: frame_stride=%lld is below pitch * (H - 1) + W = %lld", a.frame_stride, (long long)a.pitch * (H - 1) + W);
    return 0;
}
// Host planes -> d_u8, packed tight on the way (frame b: H rows of W luma bytes, then H / 2 rows of W chroma bytes; 1.5 bytes a pixel).
// Only bytes [0, W) of a row are read: planes at pitch W are uploaded as they lie, wider ones are packed row by row on the host first.
int upload_nv12(hp3d_ctx* ctx, int B, int H, int W, const Nv12Arg& a, Nv12Src* out) {
    const size_t ny = (size_t)H * W, nc = (size_t)(H / 2) * W, fs = ny + nc, nbytes = fs * B;
    if (nbytes > ctx->u8_bytes) { CHK(dev_realloc(ctx, &ctx->d_u8, nbytes)); ctx->u8_bytes = nbytes; }
    const size_t stride = B > 1 ? (size_t)a.frame_stride : 0;
    if (a.pitch == W) {
        for (int b = 0; b < B; ++b) {
            HIPCHK(ctx, hipMemcpyAsync(ctx->d_u8 + b * fs, a.y + b * stride, ny, hipMemcpyHostToDevice, ctx->stream));
            HIPCHK(ctx, hipMemcpyAsync(ctx->d_u8 + b * fs + ny, a.uv + b * stride, nc, hipMemcpyHostToDevice, ctx->stream));
        }
    } else {
        // (the previous call's upload has completed: every host form ends on a stream synchronise)
        ctx->h_nv12.resize(nbytes);
        for (int b = 0; b < B; ++b) {
            unsigned char* d = ctx->h_nv12.data() + b * fs;
            for (int r = 0; r < H; ++r) memcpy(d + (size_t)r * W, a.y + b * stride + (size_t)r * a.pitch, W);
            for (int r = 0; r < H / 2; ++r) memcpy(d + ny + (size_t)r * W, a.uv + b * stride + (size_t)r * a.pitch, W);
        }
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_u8, ctx->h_nv12.data(), nbytes, hipMemcpyHostToDevice, ctx->stream));
    }
    *out = nv12_src(ctx->d_u8, ctx->d_u8 + ny, W, fs, ctx->nv12_matrix);
    return 0;
}

// ---- packed 8-bit frames (layout and formats: include/hp3d.h) ---------------------------------------------------------
// What the caller handed over: frame 0's first byte (host or device pointer), the row pitch, the frame stride, the format.
struct PxArg {
    const unsigned char* px;
    int pitch;
    long long frame_stride;
    int format;
};
// every refusal comes before anything is enqueued
int check_px(hp3d_ctx* ctx, int B, int H, int W, const PxArg& a) {
    const int pb = px_pixel_bytes(a.format);
    if (!pb) HP3D_FAIL(ctx, HP3D_ERR_ARG, "px: format=%d is none of HP3D_PX_RGB ... HP3D_PX_ABGR (0 ... 5)", a.format);
    if (!a.px) HP3D_FAIL(ctx, HP3D_ERR_ARG, "px: px (the surface) is NULL");
    if (B < 1 || H < 16 || W < 16) HP3D_FAIL(ctx, HP3D_ERR_ARG, "bad shape B=%d H=%d W=%d (need B>=1, H,W >=16)", B, H, W);
    if (a.pitch < (long long)W * pb) HP3D_FAIL(ctx, HP3D_ERR_ARG, "px: pitch=%d is below W * pixel_bytes = %lld", a.pitch, (long long)W * pb);
    const long long need = (long long)a.pitch * (H - 1) + (long long)W * pb;
    if (B > 1 && a.frame_stride < need)
        HP3D_FAIL(ctx, HP3D_ERR_ARG, "px: frame_stride=%lld is below pitch * (H - 1) + W * pixel_bytes = %lld", a.frame_stride, need);
    return 0;
}
// Host frames -> d_u8, packed tight at pixel_bytes bytes a pixel (the buffer is sized for 4: a stream that changes format re-allocates
// nothing).  Only bytes [0, W pixel_bytes) of a row are read: contiguous rows and frames are ONE copy as they lie, anything else is
// packed row by row on the host first.  A 4-byte surface always lands `wide`; the 4-to-3 gather is the kernels' job.
int upload_px(hp3d_ctx* ctx, int B, int H, int W, const PxArg& a, PxSrc* out) {
    const int pb = px_pixel_bytes(a.format);
    const size_t row = (size_t)W * pb, fs = row * H, nbytes = fs * B, cap = (size_t)B * H * W * 4;
    if (cap > ctx->u8_bytes) { CHK(dev_realloc(ctx, &ctx->d_u8, cap)); ctx->u8_bytes = cap; }
    const size_t stride = B > 1 ? (size_t)a.frame_stride : 0;
    if ((size_t)a.pitch == row && (B == 1 || stride == fs)) {
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_u8, a.px, nbytes, hipMemcpyHostToDevice, ctx->stream));
    } else {
        // (the previous call's upload has completed: every host form ends on a stream synchronise)
        ctx->h_px.resize(nbytes);
        for (int b = 0; b < B; ++b)
            for (int r = 0; r < H; ++r) memcpy(ctx->h_px.data() + b * fs + r * row, a.px + b * stride + (size_t)r * a.pitch, row);
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_u8, ctx->h_px.data(), nbytes, hipMemcpyHostToDevice, ctx->stream));
    }
    *out = px_src(ctx->d_u8, (int)row, B > 1 ? fs : 0, a.format);
    return 0;
}

// ---- a batch of separate surfaces, formats mixed (the record: include/hp3d.h) -----------------------------------------
static_assert(HP3D_SURF_FORMAT_NV12 == HP3D_SURF_NV12, "hp3d_common.h and include/hp3d.h disagree");
static_assert(sizeof(SurfRec) % sizeof(int) == 0, "the staging buffers count in ints");
// the bytes of the picture in a row of surface s (0: unknown format)
static size_t surf_row_bytes(const hp3d_surface& s, int W) {
    return s.format == HP3D_SURF_NV12 ? (size_t)W : (size_t)W * px_pixel_bytes(s.format);
}
// every refusal comes before anything is enqueued and names the surface
int check_surfaces(hp3d_ctx* ctx, int B, int H, int W, const hp3d_surface* sf) {
    if (!sf) HP3D_FAIL(ctx, HP3D_ERR_ARG, "surf: surfaces is NULL");
    if (B < 1 || H < 16 || W < 16) HP3D_FAIL(ctx, HP3D_ERR_ARG, "bad shape B=%d H=%d W=%d (need B>=1, H,W >=16)", B, H, W);
    for (int i = 0; i < B; ++i) {
        const hp3d_surface& s = sf[i];
        const bool nv = s.format == HP3D_SURF_NV12;
        if (!nv && !px_pixel_bytes(s.format))
            HP3D_FAIL(ctx, HP3D_ERR_ARG, "surf: surfaces[%d].format=%d is none of HP3D_PX_RGB ... HP3D_PX_ABGR (0 ... 5) or HP3D_SURF_NV12 (16)", i,
                      (int)s.format);
        if (!s.data) HP3D_FAIL(ctx, HP3D_ERR_ARG, "surf: surfaces[%d].data is NULL", i);
        if (nv && !s.chroma) HP3D_FAIL(ctx, HP3D_ERR_ARG, "surf: surfaces[%d].chroma is NULL on an NV12 surface", i);
        if (!nv && s.chroma) HP3D_FAIL(ctx, HP3D_ERR_ARG, "surf: surfaces[%d].chroma must be NULL on a packed format (format=%d)", i, (int)s.format);
        if (s.height != H || s.width != W)
            HP3D_FAIL(ctx, HP3D_ERR_ARG, "surf: surfaces[%d] is %dx%d, the call is %dx%d: mixed sizes are not supported yet", i, (int)s.height,
                      (int)s.width, H, W);
        if (nv && ((H | W) & 1))
            HP3D_FAIL(ctx, HP3D_ERR_ARG, "surf: surfaces[%d] is NV12: H=%d and W=%d must be even (a chroma sample covers 2 x 2 pixels)", i, H, W);
        if ((long long)s.pitch < (long long)surf_row_bytes(s, W))
            HP3D_FAIL(ctx, HP3D_ERR_ARG, "surf: surfaces[%d].pitch=%d is below the row's %lld bytes", i, (int)s.pitch, (long long)surf_row_bytes(s, W));
    }
    return 0;
}
int ensure_surf(hp3d_ctx* ctx, int B) {
    SurfTable& Q = ctx->surf;
    if (B <= Q.cap) return 0;
    for (HostFlags& h : Q.stage) CHK(h.wait(ctx));
    CHK(dev_realloc(ctx, &Q.d_rec, (size_t)B));
    for (HostFlags& h : Q.stage) CHK(h.resize(ctx, (size_t)B * (sizeof(SurfRec) / sizeof(int)), "surface table"));
    Q.cap = B;
    return 0;
}
void surf_free(hp3d_ctx* ctx) {
    SurfTable& Q = ctx->surf;
    if (Q.d_rec) hipFree(Q.d_rec);
    for (HostFlags& h : Q.stage) h.free();
    Q = SurfTable();
}
// The table of a call: *h = B records of page-locked staging to fill (surf_rec, from DEVICE addresses), then surf_table_commit copies
// them to the device table behind the stream.  The staging buffers take turns and each is rewritten only after the event behind its
// last copy: that copy belongs to the call before the previous one, so the wait holds the host only when it runs two calls ahead of the
// device -- an event wait, never a stream synchronise.  (A tracker's wait for the previous step's flags orders the copy of every step
// but the one behind a reset, a failed step or a per-op call; the second buffer makes the rule hold without that case analysis.)
int surf_table_begin(hp3d_ctx* ctx, int B, SurfRec** h) {
    CHK(ensure_surf(ctx, B));
    HostFlags& st = ctx->surf.stage[ctx->surf.turn];
    CHK(st.wait(ctx));
    *h = (SurfRec*)st.h;
    return 0;
}
int surf_table_commit(hp3d_ctx* ctx, int B, SurfSrc* out) {
    SurfTable& Q = ctx->surf;
    HostFlags& st = Q.stage[Q.turn];
    Q.turn ^= 1;
    HIPCHK(ctx, hipMemcpyAsync(Q.d_rec, st.h, sizeof(SurfRec) * (size_t)B, hipMemcpyHostToDevice, ctx->stream));
    CHK(st.record(ctx));
    *out = surf_src(Q.d_rec, ctx->nv12_matrix);
    return 0;
}
// device surfaces: the records from the caller's addresses, in place
int surf_table_dev(hp3d_ctx* ctx, int B, const hp3d_surface* sf, SurfSrc* out) {
    SurfRec* h;
    CHK(surf_table_begin(ctx, B, &h));
    for (int b = 0; b < B; ++b) h[b] = surf_rec(sf[b].data, sf[b].chroma, sf[b].pitch, sf[b].format);
    return surf_table_commit(ctx, B, out);
}
// Host surfaces -> d_u8, each packed tight into a slot of its own (4 H W bytes rounded up to 16: a 4-byte surface lands `wide`, and a
// stream that changes format re-allocates nothing), as upload_px / upload_nv12 pack theirs: one copy where the rows are contiguous, row
// by row through h_px otherwise.  Only the picture's bytes of a row are read.  The table is built over the upload.
int upload_surf(hp3d_ctx* ctx, int B, int H, int W, const hp3d_surface* sf, SurfSrc* out) {
    const size_t slot = ((size_t)H * W * 4 + 15) / 16 * 16, cap = slot * B, ny = (size_t)H * W;
    if (cap > ctx->u8_bytes) { CHK(dev_realloc(ctx, &ctx->d_u8, cap)); ctx->u8_bytes = cap; }
    // (the previous call's upload has completed: every host form ends on a stream synchronise)
    size_t packed = 0;
    for (int b = 0; b < B; ++b)
        if ((size_t)sf[b].pitch != surf_row_bytes(sf[b], W)) packed += sf[b].format == HP3D_SURF_NV12 ? ny + ny / 2 : surf_row_bytes(sf[b], W) * H;
    ctx->h_px.resize(packed);
    unsigned char* hp = ctx->h_px.data();
    SurfRec* h;
    CHK(surf_table_begin(ctx, B, &h));
    for (int b = 0; b < B; ++b) {
        const hp3d_surface& s = sf[b];
        const size_t row = surf_row_bytes(s, W);
        unsigned char* d = ctx->d_u8 + b * slot;
        const bool nv = s.format == HP3D_SURF_NV12;
        if ((size_t)s.pitch == row) {
            HIPCHK(ctx, hipMemcpyAsync(d, s.data, row * H, hipMemcpyHostToDevice, ctx->stream));
            if (nv) HIPCHK(ctx, hipMemcpyAsync(d + ny, s.chroma, ny / 2, hipMemcpyHostToDevice, ctx->stream));
        } else {
            const size_t n = nv ? ny + ny / 2 : row * H;
            for (int r = 0; r < H; ++r) memcpy(hp + (size_t)r * row, s.data + (size_t)r * s.pitch, row);
            for (int r = 0; nv && r < H / 2; ++r) memcpy(hp + ny + (size_t)r * row, s.chroma + (size_t)r * s.pitch, row);
            HIPCHK(ctx, hipMemcpyAsync(d, hp, n, hipMemcpyHostToDevice, ctx->stream));
            hp += n;
        }
        h[b] = surf_rec(d, nv ? d + ny : nullptr, (int)row, s.format);
    }
    return surf_table_commit(ctx, B, out);
}
// mean bytes a pixel of the surfaces (the profile rows' traffic figure)
static double surf_mean_bpp(int B, const hp3d_surface* sf) {
    double b = 0;
    for (int i = 0; i < B; ++i) b += sf[i].format == HP3D_SURF_NV12 ? 1.5 : px_pixel_bytes(sf[i].format);
    return b / B;
}

// The frames of a chunk of a tracking step: float32, uint8, NV12, packed 8-bit or separate surfaces -- exactly one is set.  The wrappers
// below switch on the kind, so the branch is written once; the float32 and uint8 launches, profile rows and counters are the ones they
// were.
struct FrameSrc {
    const float* f32 = nullptr;
    const unsigned char* u8 = nullptr;
    const Nv12Src* nv12 = nullptr;
    const PxSrc* px = nullptr;
    const SurfSrc* surf = nullptr;
    double surf_bpp = 0;                  // surf: mean bytes a pixel of the step's surfaces
    bool raw() const { return u8 || nv12 || px || surf; }
};
// the nb * K crops of nb frames, K boxes per frame, into d_crop
int crop_frames(hp3d_ctx* ctx, const FrameSrc& src, int nb, int K, int H, int W, const float* bc, const float* bs) {
    const int ns = nb * K;
    if (src.surf) {
        ProfScope ps(ctx, "crop_and_resize_surf", "crop_and_resize_surf", 0.0, src.surf_bpp * nb * H * W + 4.0 * ns * 256 * 256 * 3);
        crop_and_resize_surf_launch(*src.surf, ns, H, W, bc, bs, nullptr, K, 256, ctx->d_crop, ctx->stream);
        ++ctx->crop_surf_launches;
    } else if (src.px) {
        ProfScope ps(ctx, "crop_and_resize_px", "crop_and_resize_px", 0.0, (double)src.px->pixel_bytes * nb * H * W + 4.0 * ns * 256 * 256 * 3);
        crop_and_resize_px_launch(*src.px, ns, H, W, bc, bs, nullptr, K, 256, ctx->d_crop, ctx->stream);
        ++ctx->crop_px_launches;
    } else if (src.nv12) {
        ProfScope ps(ctx, "crop_and_resize_nv12", "crop_and_resize_nv12", 0.0, 1.5 * nb * H * W + 4.0 * ns * 256 * 256 * 3);
        crop_and_resize_nv12_launch(*src.nv12, ns, H, W, bc, bs, nullptr, K, 256, ctx->d_crop, ctx->stream);
        ++ctx->crop_nv12_launches;
    } else if (src.u8) {          // the crop comes from the frame itself: no normalised full-size frame exists
        ProfScope ps(ctx, "crop_and_resize_u8", "crop_and_resize_u8", 0.0, 1.0 * nb * H * W * 3 + 4.0 * ns * 256 * 256 * 3);
        crop_and_resize_u8_launch(src.u8, ns, H, W, bc, bs, 256, ctx->d_crop, ctx->stream, K);
        ++ctx->crop_u8_launches;
    } else {
        ProfScope ps(ctx, "crop_and_resize", "crop_and_resize", 0.0, 4.0 * nb * (H * W * 3 + K * 256 * 256 * 3));
        crop_and_resize_launch(src.f32, ns, H, W, 3, bc, bs, 256, ctx->d_crop, ctx->stream, K);
    }
    HIPCHK(ctx, hipGetLastError());
    return 0;
}
// the m crops of the slots idx[i] (option "hands_compact"), dense, into d_crop
int crop_frames_idx(hp3d_ctx* ctx, const FrameSrc& src, int nb, int K, int H, int W, const float* center, const float* scale, const int* d_idx,
                    int m) {
    if (src.surf) {
        ProfScope ps(ctx, "crop_and_resize_idx_surf", "crop_and_resize_idx_surf", 0.0, src.surf_bpp * nb * H * W + 4.0 * m * 256 * 256 * 3);
        crop_and_resize_surf_launch(*src.surf, m, H, W, center, scale, d_idx, K, 256, ctx->d_crop, ctx->stream);
        ++ctx->crop_surf_launches;
    } else if (src.px) {
        ProfScope ps(ctx, "crop_and_resize_idx_px", "crop_and_resize_idx_px", 0.0, (double)src.px->pixel_bytes * nb * H * W + 4.0 * m * 256 * 256 * 3);
        crop_and_resize_px_launch(*src.px, m, H, W, center, scale, d_idx, K, 256, ctx->d_crop, ctx->stream);
        ++ctx->crop_px_launches;
    } else if (src.nv12) {
        ProfScope ps(ctx, "crop_and_resize_idx_nv12", "crop_and_resize_idx_nv12", 0.0, 1.5 * nb * H * W + 4.0 * m * 256 * 256 * 3);
        crop_and_resize_nv12_launch(*src.nv12, m, H, W, center, scale, d_idx, K, 256, ctx->d_crop, ctx->stream);
        ++ctx->crop_nv12_launches;
    } else if (src.u8) {
        ProfScope ps(ctx, "crop_and_resize_idx_u8", "crop_and_resize_idx_u8", 0.0, 1.0 * nb * H * W * 3 + 4.0 * m * 256 * 256 * 3);
        crop_and_resize_idx_u8_launch(src.u8, m, H, W, center, scale, d_idx, K, 256, ctx->d_crop, ctx->stream);
        ++ctx->crop_u8_launches;
    } else {
        ProfScope ps(ctx, "crop_and_resize_idx", "crop_and_resize_idx", 0.0, 4.0 * ((double)nb * H * W * 3 + (double)m * 256 * 256 * 3));
        crop_and_resize_idx_launch(src.f32, m, H, W, 3, center, scale, d_idx, K, 256, ctx->d_crop, ctx->stream);
    }
    HIPCHK(ctx, hipGetLastError());
    return 0;
}
// a raw frame as the normalised float32 frame in d_image: all nb frames (idx null) or the frames idx[i], i < nb, dense
int normalise_frames(hp3d_ctx* ctx, const FrameSrc& src, const int* idx, int nb, int H, int W) {
    if (src.surf) {
        const char* row = idx ? "preprocess_surf_idx" : "preprocess_surf";
        ProfScope ps(ctx, row, row, 0.0, src.surf_bpp * nb * H * W + 4.0 * nb * H * W * 3);
        downscale_surf_launch(*src.surf, idx, nb, H, W, 1, ctx->d_image, ctx->stream);
    } else if (src.px) {
        const char* row = idx ? "preprocess_px_idx" : "preprocess_px";
        ProfScope ps(ctx, row, row, 0.0, (double)src.px->pixel_bytes * nb * H * W + 4.0 * nb * H * W * 3);
        downscale_px_launch(*src.px, idx, nb, H, W, 1, ctx->d_image, ctx->stream);
    } else if (src.nv12) {
        const char* row = idx ? "preprocess_nv12_idx" : "preprocess_nv12";
        ProfScope ps(ctx, row, row, 0.0, 1.5 * nb * H * W + 4.0 * nb * H * W * 3);
        downscale_nv12_launch(*src.nv12, idx, nb, H, W, 1, ctx->d_image, ctx->stream);
    } else if (idx) {
        ProfScope ps(ctx, "preprocess_u8_idx", "preprocess_u8_idx", 0.0, 5.0 * nb * H * W * 3);
        preprocess_u8_idx_launch(src.u8, idx, nb, H, W, ctx->d_image, ctx->stream);
    } else {
        ProfScope ps(ctx, "preprocess_u8", "preprocess_u8", 0.0, 1.0 * nb * H * W * 3 + 4.0 * nb * H * W * 3);
        preprocess_u8_launch(src.u8, nb, H, W, H, W, ctx->d_image, ctx->stream);
    }
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

// the front of such a detect step: the detection frame into d_image, detection at (nb, Hd, Wd), the boxes of `slots` slots to the frame
// idx (option "track_partial_detect", K = 0): nb = the number of frames that detect, frame i of them is the source's frame idx[i]; the
// boxes come out dense
int run_detect_reduced(hp3d_ctx* ctx, const FrameSrc& src, int nb, int H, int W, int Hd, int Wd, int K = 0,
                       const MaskKeep& mk = MaskKeep(), const int* idx = nullptr) {
    const int f = ctx->detect_scale, slots = nb * std::max(K, 1);
    const float* d_img = src.f32;
    const unsigned char* d_u8 = src.u8;
    if (src.surf) {
        const char* row = idx ? "downscale_surf_idx" : "downscale_surf";
        ProfScope ps(ctx, row, row, 0.0, src.surf_bpp * nb * H * W + 4.0 * nb * Hd * Wd * 3);
        downscale_surf_launch(*src.surf, idx, nb, H, W, f, ctx->d_image, ctx->stream);
        HIPCHK(ctx, hipGetLastError());
    } else if (src.px) {
        const char* row = idx ? "downscale_px_idx" : "downscale_px";
        ProfScope ps(ctx, row, row, 0.0, (double)src.px->pixel_bytes * nb * H * W + 4.0 * nb * Hd * Wd * 3);
        downscale_px_launch(*src.px, idx, nb, H, W, f, ctx->d_image, ctx->stream);
        HIPCHK(ctx, hipGetLastError());
    } else if (src.nv12) {
        const char* row = idx ? "downscale_nv12_idx" : "downscale_nv12";
        ProfScope ps(ctx, row, row, 0.0, 1.5 * nb * H * W + 4.0 * nb * Hd * Wd * 3);
        downscale_nv12_launch(*src.nv12, idx, nb, H, W, f, ctx->d_image, ctx->stream);
        HIPCHK(ctx, hipGetLastError());
    } else if (idx) {
        const char* row = d_u8 ? "downscale_u8_idx" : "downscale_idx";
        ProfScope ps(ctx, row, row, 0.0, (double)nb * H * W * 3 * (d_u8 ? 1.0 : 4.0) + 4.0 * nb * Hd * Wd * 3);
        if (d_u8) downscale_u8_idx_launch(d_u8, idx, nb, H, W, f, ctx->d_image, ctx->stream);
        else downscale_idx_launch(d_img, idx, nb, H, W, f, ctx->d_image, ctx->stream);
        HIPCHK(ctx, hipGetLastError());
    } else {
        const double px = (double)nb * H * W * 3;
        ProfScope ps(ctx, d_u8 ? "downscale_u8" : "downscale", d_u8 ? "downscale_u8" : "downscale", 0.0, px * (d_u8 ? 1.0 : 4.0) + 4.0 * nb * Hd * Wd * 3);
        if (d_u8) downscale_u8_launch(d_u8, nb, H, W, f, ctx->d_image, ctx->stream);
        else downscale_launch(d_img, nb, H, W, f, ctx->d_image, ctx->stream);
        HIPCHK(ctx, hipGetLastError());
    }
    MaskKeep mkd = mk;
    if (K > 0 && mk.keep) {
        ProfScope ps(ctx, "box_to_detect", "box_to_detect", 0.0, 24.0 * slots);
        box_to_detect_launch(mk.center, mk.scale, slots, f, ctx->d_keepc, ctx->d_keeps, ctx->stream);
        mkd.center = ctx->d_keepc; mkd.scale = ctx->d_keeps;
    }
    CHK(run_detect_and_crop(ctx, ctx->d_image, nb, Hd, Wd, 0, true, false, K, mkd));
    ProfScope ps(ctx, "box_to_frame", "box_to_frame", 0.0, 28.0 * slots);
    box_to_frame_launch(ctx->d_center, ctx->d_cropsize, slots, f, ctx->d_center, ctx->d_cropsize, ctx->d_scale, ctx->stream);
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

// ---- what the step functions share (hp3d_track_step*, hp3d_track_hands_step*, hp3d_infer_hands*) ----------------------------------
// What a step was handed: the frames -- float32, uint8 (host), NV12 or packed 8-bit, exactly one is set -- and hand_side; dev: device
// pointers.
struct StepIn {
    const float* image = nullptr;
    const unsigned char* image_u8 = nullptr;
    const Nv12Arg* nv = nullptr;
    const float* hand_side = nullptr;
    bool dev = false;
    const PxArg* px = nullptr;
    const hp3d_surface* surf = nullptr;                  // B records in host memory
    bool raw() const { return image_u8 || nv || px || surf; }    // uint8, NV12, packed 8-bit frames or surfaces: no float32 frame comes in
};
// Where a step's results go, one entry per slot (null: skipped); device pointers when the step's input is.
struct StepOut {
    float *image_crop = nullptr, *scale_crop = nullptr, *center = nullptr, *kp_scoremap = nullptr, *coord3d = nullptr;
    int32_t* kp_crop = nullptr;
    double* kp_image = nullptr;
    float* confidence = nullptr;
    int32_t *lost = nullptr, *detected = nullptr, *valid = nullptr, *area = nullptr, *claimed = nullptr;
    // the outputs of the chunk that starts at slot s0
    StepOut at(size_t s0) const {
        StepOut o;
        auto off = [s0](auto* p, size_t per) { return p ? p + s0 * per : nullptr; };
        o.image_crop = off(image_crop, 256 * 256 * 3); o.scale_crop = off(scale_crop, 1); o.center = off(center, 2);
        o.kp_scoremap = off(kp_scoremap, 256 * 256 * 21); o.coord3d = off(coord3d, 63);
        o.kp_crop = off(kp_crop, 42); o.kp_image = off(kp_image, 42); o.confidence = off(confidence, 1);
        o.lost = off(lost, 1); o.detected = off(detected, 1); o.valid = off(valid, 1); o.area = off(area, 1); o.claimed = off(claimed, 1);
        return o;
    }
};
int copy_out(hp3d_ctx* ctx, int32_t* dst, const int* src, size_t n, bool dev) {          // (int32: four bytes each, as copy_out counts)
    return copy_out(ctx, (float*)dst, (const float*)src, n, dev);
}

// The frames of a tracking step on the device.  upload(), once: uint8 frames into d_u8, NV12 and packed 8-bit surfaces in place (dev) or
// as their packed upload.  chunk(), per chunk of nb frames from b0 with K slots each: hand_side and a host float32 frame to the device, then the chunk's
// FrameSrc.  stage: the host float32 frame goes to d_stage, because the chunk puts something else into d_image (a detection frame, the
// gathered lost frames).
struct StepFrames {
    const StepIn& in;
    const int H, W;
    Nv12Src nvs{}, nvc{};
    PxSrc pxs{}, pxc{};
    SurfSrc sfs{}, sfc{};                 // the step's table, and it from the chunk's first frame on
    double surf_bpp = 0;
    const float* d_hs = nullptr;          // the chunk's hand_side on the device
    FrameSrc src;                         // the chunk's frames (src.nv12, src.px and src.surf point into this record)
    int upload(hp3d_ctx* ctx, int B) {
        if (in.image_u8) {
            const size_t nbytes = (size_t)B * H * W * 3;
            if (nbytes > ctx->u8_bytes) { CHK(dev_realloc(ctx, &ctx->d_u8, nbytes)); ctx->u8_bytes = nbytes; }
            HIPCHK(ctx, hipMemcpyAsync(ctx->d_u8, in.image_u8, nbytes, hipMemcpyHostToDevice, ctx->stream));
        }
        if (in.nv && in.dev) nvs = nv12_src(in.nv->y, in.nv->uv, in.nv->pitch, B > 1 ? (size_t)in.nv->frame_stride : 0, ctx->nv12_matrix);
        else if (in.nv) CHK(upload_nv12(ctx, B, H, W, *in.nv, &nvs));
        if (in.px && in.dev) pxs = px_src(in.px->px, in.px->pitch, B > 1 ? (size_t)in.px->frame_stride : 0, in.px->format);
        else if (in.px) CHK(upload_px(ctx, B, H, W, *in.px, &pxs));
        if (in.surf && in.dev) CHK(surf_table_dev(ctx, B, in.surf, &sfs));
        else if (in.surf) CHK(upload_surf(ctx, B, H, W, in.surf, &sfs));
        if (in.surf) surf_bpp = surf_mean_bpp(B, in.surf);
        return 0;
    }
    int chunk(hp3d_ctx* ctx, int b0, int nb, int K, bool stage) {
        const size_t px = (size_t)H * W * 3;
        d_hs = in.hand_side + (size_t)b0 * K * 2;
        src = FrameSrc();
        src.f32 = in.image ? in.image + b0 * px : nullptr;
        src.u8 = in.image_u8 ? ctx->d_u8 + b0 * px : nullptr;
        if (!in.dev) {
            CHK(copy_in(ctx, ctx->d_hs, d_hs, (size_t)nb * K * 2, false));
            d_hs = ctx->d_hs;
            if (!in.raw()) {
                float* to = stage ? ctx->d_stage : ctx->d_image;
                CHK(copy_in(ctx, to, src.f32, nb * px, false));
                src.f32 = to;
            }
        }
        nvc = nvs.at(b0);
        src.nv12 = in.nv ? &nvc : nullptr;
        pxc = pxs.at(b0);
        src.px = in.px ? &pxc : nullptr;
        sfc = sfs.at(b0);
        src.surf = in.surf ? &sfc : nullptr;
        src.surf_bpp = surf_bpp;
        return 0;
    }
};

// frames per chunk of a multi-hand call: a chunk of the front half's size that holds at most micro_batch slots (at least one frame)
int slot_micro_batch(const hp3d_ctx* ctx, int B, int K, int H, int W) {
    const int front = auto_micro_batch(ctx, B, H, W), back = auto_micro_batch(ctx, B * K, 256, 256);
    int mb = front <= 0 ? B : std::min(front, B);
    if (back > 0) mb = std::min(mb, std::max(1, back / K));
    return mb;
}

// The boxes of a detect step's chunk: HandSegNet, the soft-max and the mask growth on the frames themselves -- a raw frame is normalised
// into d_image first, as hp3d_infer_full_u8 does -- or, at detect_scale > 1, on their area mean (run_detect_reduced).  *crop_src: what
// the crops are then taken from -- the frames, or the normalised frame where one was made (the crop is then infer_full_impl's).
int run_detect_front(hp3d_ctx* ctx, const FrameSrc& src, int nb, int H, int W, int Hd, int Wd, int K, const MaskKeep& mk, FrameSrc* crop_src) {
    *crop_src = src;
    if (ctx->detect_scale > 1) return run_detect_reduced(ctx, src, nb, H, W, Hd, Wd, K, mk);
    const bool raw = src.raw();
    if (raw) {
        CHK(normalise_frames(ctx, src, nullptr, nb, H, W));
        *crop_src = FrameSrc();
        crop_src->f32 = ctx->d_image;
    }
    return run_detect_and_crop(ctx, crop_src->f32, nb, H, W, 0, raw, false, K, mk);
}

// The back half of every step behind the n crops in d_crop: PoseNet2D, then the lifting stage with the heat-map up-sampling and the
// keypoint detection beside it (on two streams with option "lift_overlap": infer_full_impl).
struct BackHalf {
    int n;
    const float* hand_side;               // device, per slot
    const float *center, *scale;          // device: the boxes kp_detect maps the keypoints with (null: d_center / d_scale)
    float* kpmap;                         // device: where the up-sampled maps go (null: none)
    int32_t* kp_crop;                     // kp_detect's outputs as run_kp_detect takes them
    double* kp_image;
    bool dev;
    bool kp_detect;                       // the trackers: always (the next boxes come from the keypoints); hp3d_infer_hands*: when asked for
};
// after_kp: the caller's launches behind kp_detect (the trackers' box rule)
template <class F>
int run_back_half(hp3d_ctx* ctx, const BackHalf& b, F&& after_kp) {
    CHK(run_posenet(ctx, ctx->d_crop, b.n, 256, 256, true));
    const std::function<int(hipStream_t)> kp_up = [&](hipStream_t st) -> int {
        if (b.kpmap) {
            ProfScope ps(ctx, "kp_upsample", "resize_bilinear", 0.0, 4.0 * b.n * (32 * 32 * 21 + 256 * 256 * 21));
            resize_bilinear_launch(ctx->d_sm[2], b.n, 32, 32, 21, 32, 256, 256, b.kpmap, st);
        }
        return 0;
    };
    const std::function<int(hipStream_t)> kp_work = [&](hipStream_t) -> int {
        if (b.kp_detect) CHK(run_kp_detect(ctx, b.n, b.kp_crop, b.kp_image, b.dev, b.scale, b.center));
        return after_kp();
    };
    return run_pose3d(ctx, ctx->d_sm[2], b.hand_side, b.n, HP3D_VARIANT_PROPOSED, &kp_work, &kp_up);
}
// ... for a step whose caller reads the maps from `out` (a device caller) or from d_kpmap (a host caller: copy_out_slots)
BackHalf back_half_to(hp3d_ctx* ctx, const StepOut& out, int n, const float* hand_side, const float* center, const float* scale, bool dev,
                      bool kp_detect) {
    float* kpmap = !out.kp_scoremap ? nullptr : dev ? out.kp_scoremap : ctx->d_kpmap;
    return BackHalf{n, hand_side, center, scale, kpmap, out.kp_crop, out.kp_image, dev, kp_detect};
}
// image_crop, the boxes, kp_scoremap and coord3d of n slots to the caller, in infer_full_impl's order.  back = false: a compacted chunk
// has delivered crop, maps and coordinates itself.
int copy_out_slots(hp3d_ctx* ctx, const StepOut& out, int n, const float* scale, const float* center, bool dev, bool back = true) {
    if (back) CHK(copy_out(ctx, out.image_crop, ctx->d_crop, (size_t)n * 256 * 256 * 3, dev));
    CHK(copy_out(ctx, out.scale_crop, scale, (size_t)n, dev));
    CHK(copy_out(ctx, out.center, center, (size_t)n * 2, dev));
    if (back && !dev) CHK(copy_out(ctx, out.kp_scoremap, ctx->d_kpmap, (size_t)n * 256 * 256 * 21, false));
    if (back) CHK(copy_out(ctx, out.coord3d, ctx->d_coord, (size_t)n * 63, dev));
    return 0;
}

// One step of a video: a DETECT step (HandSegNet -> mask -> box for the whole batch, then per image the tracked box where it is
// still good) or a TRACKED step (no HandSegNet, no soft-max, no mask growth: the crop comes from the boxes the previous step
// derived from its keypoints).  Behind the crop both are infer_full_impl: PoseNet2D, the lifting stage, keypoint detection -- plus
// the one launch that turns the keypoints into the next boxes.  The step type is decided on the host, before anything is enqueued,
// from the previous step's `lost` flags (4 * B bytes that travel behind that step); the whole batch detects when any image is lost:
// one kernel plan per step, no gather of the lost images -- unless option "track_partial_detect" (DESIGN.md 4.16): a detect step that
// only `lost` flags caused then runs HandSegNet, the soft-max and the mask growth per chunk at batch m = the chunk's lost frames, on
// those frames (0 < m < nb: "partial"; m = 0: the chunk is enqueued as a tracked chunk; m = nb: as without the option).
// uint8 frames (host, frame = network size): the tracked step crops straight from the uint8 frame, the detect step normalises it
// first (preprocess_u8) as hp3d_infer_full_u8 does.
int track_step_impl(hp3d_ctx* ctx, int B, int H, int W, const StepIn& in, const StepOut& out) {
    if ((!in.image && !in.raw()) || !in.hand_side) HP3D_FAIL(ctx, HP3D_ERR_ARG, "image / hand_side is NULL");
    if (in.nv) CHK(check_nv12(ctx, B, H, W, *in.nv));
    if (in.px) CHK(check_px(ctx, B, H, W, *in.px));
    if (in.surf) CHK(check_surfaces(ctx, B, H, W, in.surf));
    CHK(check_img(ctx, B, H, W));
    const bool dev = in.dev;
    int Hd, Wd;
    CHK(detect_frame(ctx, H, W, &Hd, &Wd));
    const int f = ctx->detect_scale;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    TrackState& T = ctx->track;
    CHK(T.h_lost.wait(ctx));                             // the only wait tracking adds: the previous step's flags
    const bool fresh = !T.valid || T.B != B || T.H != H || T.W != W || T.f != f;
    bool any_lost = false;
    if (!fresh)
        for (int b = 0; b < B; ++b) any_lost = any_lost || T.h_lost.h[b] != 0;
    const bool sched = ctx->track_redetect > 0 && T.since + 1 >= ctx->track_redetect;
    const bool detect = fresh || any_lost || sched;
    const int force_all = (fresh || sched) ? 1 : 0;      // nothing to keep / a scheduled re-detection re-boxes every image
    CHK(need_nets(ctx, (detect ? NET_SEG : 0) | NET_POSE | NET_PRIOR | NET_VP));
    const int mb0 = auto_micro_batch(ctx, B, Hd, Wd);
    const int mb = mb0 <= 0 ? B : std::min(mb0, B);
    CHK(ensure_arena(ctx, mb, Hd, Wd));
    // option "track_partial_detect": only a detect step that `lost` flags alone caused (a fresh or scheduled one re-boxes every image)
    const bool partial_step = ctx->track_partial_detect && detect && !force_all;
    // a host float32 frame is staged where the detection frame (f > 1) or the gathered lost frames (a partial chunk) go to d_image
    if ((f > 1 || partial_step) && !dev && !in.raw()) CHK(ensure_stage(ctx, (size_t)mb * H * W * 3));
    CHK(ensure_track(ctx, B));
    T.valid = false;                                     // a step that fails half way leaves no boxes behind
    StepFrames fr{in, H, W};
    CHK(fr.upload(ctx, B));
    ProfCall prof(ctx);
    const int cur = T.cur, nxt = T.cur ^ 1;
    for (int b0 = 0; b0 < B; b0 += mb) {
        const int nb = std::min(mb, B - b0);
        prof.chunk(b0);
        int m = nb;                                      // the chunk's frames that detect
        if (partial_step) {
            m = 0;
            for (int b = b0; b < b0 + nb; ++b) m += T.h_lost.h[b] != 0 ? 1 : 0;
        }
        const bool partial = partial_step && m > 0 && m < nb;
        const bool chunk_detect = detect && m > 0;       // (m = 0: another chunk holds the lost frame; this one runs as a tracked chunk)
        CHK(fr.chunk(ctx, b0, nb, 1, f > 1 || partial));
        const FrameSrc& src = fr.src;
        FrameSrc crop_src = src;
        float* bc = T.center[cur] + (size_t)b0 * 2;
        float* bs = T.scale[cur] + b0;
        if (partial) {           // idx / pos from the flags, which this chunk's track_box has not overwritten yet
            int* pidx = T.pidx + b0;
            int* ppos = T.ppos + b0;
            {
                ProfScope ps(ctx, "track_partial_index", "track_partial_index", 0.0, 12.0 * nb);
                track_partial_index_launch(T.lost + b0, nb, pidx, ppos, ctx->stream);
            }
            ctx->track_partial_frames_run += m;
            ctx->track_partial_frames_skipped += nb - m;
            // the m lost frames, dense, into d_image: never the buffer the chunk's frames lie in (a host frame was staged in d_stage)
            if (f > 1) {
                CHK(run_detect_reduced(ctx, src, m, H, W, Hd, Wd, 0, MaskKeep(), pidx));
            } else {
                if (in.raw()) {
                    CHK(normalise_frames(ctx, src, pidx, m, H, W));
                } else {
                    ProfScope ps(ctx, "frame_gather", "frame_gather", 0.0, 8.0 * m * H * W * 3);
                    frame_gather_launch(src.f32, pidx, m, (size_t)H * W * 3, ctx->d_image, ctx->stream);
                    ++ctx->frame_gather_launches;
                }
                HIPCHK(ctx, hipGetLastError());
                CHK(run_detect_and_crop(ctx, ctx->d_image, m, H, W, 0, true, false));
            }
            ProfScope ps(ctx, "track_select_pos", "track_select_pos", 0.0, 16.0 * nb);
            track_select_pos_launch(T.lost + b0, ppos, ctx->d_center, ctx->d_scale, nb, bc, bs, T.detected + b0, ctx->stream);
            // (a raw frame: all nb crops straight from it = normalise, then crop, bit for bit)
        } else if (chunk_detect) {
            CHK(run_detect_front(ctx, src, nb, H, W, Hd, Wd, 0, MaskKeep(), &crop_src));
            ProfScope ps(ctx, "track_select", "track_select", 0.0, 16.0 * nb);
            track_select_launch(T.lost + b0, ctx->d_center, ctx->d_scale, nb, force_all, bc, bs, T.detected + b0, ctx->stream);
        }
        CHK(crop_frames(ctx, crop_src, nb, 1, H, W, bc, bs));
        const StepOut o = out.at(b0);
        CHK(run_back_half(ctx, back_half_to(ctx, o, nb, fr.d_hs, bc, bs, dev, true), [&]() -> int {
            ProfScope ps(ctx, "track_box", "track_box", 0.0, 4.0 * nb * 32 * 32 * 21);
            track_box_launch(dev && o.kp_image ? o.kp_image : ctx->d_kpimg, ctx->d_sm[2], 32, nb, H, W, 256, ctx->track_margin, ctx->track_min_score,
                             ctx->track_use_min_score, T.center[nxt] + (size_t)b0 * 2, T.scale[nxt] + b0, T.conf + b0, T.lost + b0,
                             chunk_detect ? nullptr : T.detected + b0, ctx->stream);
            return 0;
        }));
        CHK(copy_out_slots(ctx, o, nb, bs, bc, dev));
        CHK(copy_out(ctx, o.confidence, T.conf + b0, (size_t)nb, dev));
        CHK(copy_out(ctx, o.lost, T.lost + b0, (size_t)nb, dev));
        CHK(copy_out(ctx, o.detected, T.detected + b0, (size_t)nb, dev));
    }
    CHK(T.h_lost.copy_behind(ctx, T.lost, (size_t)B));
    T.cur = nxt; T.valid = true; T.B = B; T.H = H; T.W = W; T.f = f;
    T.since = detect ? 0 : T.since + 1;
    ++(detect ? ctx->track_detect_steps : ctx->track_tracked_steps);
    if (detect && f > 1) ++ctx->detect_scale_steps;
    if (!dev) return finish_op(ctx);
    return 0;
}

// ---- compaction of absent hand slots (option "hands_compact") ---------------------------------------------------------
int ensure_compact(hp3d_ctx* ctx, int ns) {
    CompactBufs& Q = ctx->compact;
    if (ns <= Q.cap) return 0;
    for (HostFlags& h : Q.map) CHK(h.wait(ctx));
    CHK(dev_realloc(ctx, &Q.d_map, (size_t)ns * 2));
    CHK(dev_realloc(ctx, &Q.d_hs, (size_t)ns * 2));
    CHK(dev_realloc(ctx, &Q.d_center, (size_t)ns * 2));
    CHK(dev_realloc(ctx, &Q.d_scale, (size_t)ns));
    for (HostFlags* h : {&Q.map[0], &Q.map[1], &Q.valid}) CHK(h->resize(ctx, (size_t)ns * 2, "hands_compact"));
    Q.cap = ns;
    return 0;
}

void compact_free(hp3d_ctx* ctx) {
    CompactBufs& Q = ctx->compact;
    for (void* p : {(void*)Q.d_map, (void*)Q.d_hs, (void*)Q.d_center, (void*)Q.d_scale})
        if (p) hipFree(p);
    for (HostFlags* h : {&Q.map[0], &Q.map[1], &Q.valid}) h->free();
    Q = CompactBufs();
}

// A chunk's valid flags on the host, where only the device has them (detect steps, hp3d_infer_hands*): one small copy and one stream
// synchronise, behind a HandSegNet pass (the only wait that "hands_compact_waits" counts).  Tracked steps never come here: the
// state's flags are on the host already.
int compact_wait_flags(hp3d_ctx* ctx, const int* d_valid, int ns, const int** h_valid) {
    CHK(ensure_compact(ctx, ns));
    HIPCHK(ctx, hipMemcpyAsync(ctx->compact.valid.h, d_valid, sizeof(int) * (size_t)ns, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ++ctx->hands_compact_waits;
    *h_valid = ctx->compact.valid.h;
    return 0;
}

// One chunk of a multi-hand call behind its boxes: what the compacted back half needs to know.
struct CompactChunk {
    int nb, K, H, W;
    const int* h_valid;                  // host: the chunk's nb * K flags
    FrameSrc src;                        // what the crops are taken from
    const float *center, *scale, *hand_side;      // device, slot layout
    StepOut out;                         // the chunk's outputs, slot layout: image_crop, kp_scoremap, coord3d, kp_crop and kp_image are written here
    bool dev;
    bool want_kp;                        // run kp_detect (hp3d_infer_hands*: only when asked for; the tracker: always)
    // the multi-hand tracker's box step (null: hp3d_infer_hands*): the chunk's slice of the state
    const std::function<void(const double* kp_image_dense, const int* pos)>* box = nullptr;
};

// The back half at batch m = the chunk's valid slots.  *compacted = false (m = ns: no absent slot): nothing is enqueued, the caller
// takes the uncompacted path.  Otherwise: idx / pos upload, gather, indexed crop, PoseNet2D / lifting / up-sampling / kp_detect at batch
// m (nothing of it when m = 0), the tracker's box step, and the scatter into the caller's buffers (dev) or into a staging area in bufA
// -- free once the lifting stage is enqueued -- that is then copied out.  image_crop, kp_scoremap, coord3d, kp_crop and kp_image of
// the chunk are complete behind it; the caller copies out the rest as without the option.
int run_compact_back_half(hp3d_ctx* ctx, const CompactChunk& c, bool* compacted) {
    const int ns = c.nb * c.K;
    int m = 0;
    for (int s = 0; s < ns; ++s) m += c.h_valid[s] != 0;
    ctx->hands_compact_slots_run += m;
    ctx->hands_compact_slots_skipped += ns - m;
    *compacted = m < ns;
    if (m == ns) return 0;
    CHK(ensure_compact(ctx, ns));
    CompactBufs& Q = ctx->compact;
    HostFlags& map = Q.map[Q.turn];
    Q.turn ^= 1;
    // (an event wait on the upload of two compacted chunks ago, not a stream synchronise and not counted: it can hold the host only in
    //  a call of three or more compacted chunks that runs ahead of the device by two of them; ensure_compact waits likewise when the
    //  slot count grows)
    CHK(map.wait(ctx));
    int* idx = map.h;
    int* pos = idx + ns;
    for (int s = 0, i = 0; s < ns; ++s) {
        pos[s] = c.h_valid[s] ? i : -1;
        if (c.h_valid[s]) idx[i++] = s;
    }
    for (int i = m; i < ns; ++i) idx[i] = 0;
    HIPCHK(ctx, hipMemcpyAsync(Q.d_map, idx, sizeof(int) * (size_t)ns * 2, hipMemcpyHostToDevice, ctx->stream));
    CHK(map.record(ctx));
    const int* d_idx = Q.d_map;
    const int* d_pos = Q.d_map + ns;
    if (m > 0) {
        {
            ProfScope ps(ctx, "slot_gather", "slot_gather", 0.0, 24.0 * m);
            slot_gather_launch(d_idx, m, c.hand_side, c.center, c.scale, Q.d_hs, Q.d_center, Q.d_scale, ctx->stream);
        }
        CHK(crop_frames_idx(ctx, c.src, c.nb, c.K, c.H, c.W, c.center, c.scale, d_idx, m));
        // (the dense maps and keypoints stay in d_kpmap / d_kpcrop / d_kpimg: the scatter below takes them to the caller)
        const BackHalf b{m, Q.d_hs, Q.d_center, Q.d_scale, c.out.kp_scoremap ? ctx->d_kpmap : nullptr, nullptr, nullptr, true, c.want_kp};
        CHK(run_back_half(ctx, b, [&]() -> int {
            if (c.box) (*c.box)(ctx->d_kpimg, d_pos);
            return 0;
        }));
    } else if (c.box) {
        (*c.box)(ctx->d_kpimg, d_pos);
    }
    // dense -> slot layout.  Host forms: a staging area in bufA (ns * 24 * 65536 floats and the small arrays; bufA holds 64 * 65536 per slot)
    float* st = ctx->bufA;
    auto stage = [&](size_t words) { float* p = st; st += (words + 3) & ~(size_t)3; return p; };
    float* s_crop = stage((size_t)ns * 256 * 256 * 3);
    float* s_kpmap = stage((size_t)ns * 256 * 256 * 21);
    float* s_coord = stage((size_t)ns * 63);
    float* s_kpcrop = stage((size_t)ns * 42);
    float* s_kpimg = stage((size_t)ns * 84);
    const StepOut& o = c.out;
    ScatterPlan plan;
    plan.add(ctx->d_crop, o.image_crop ? (c.dev ? o.image_crop : s_crop) : nullptr, 256 * 256 * 3);
    plan.add(ctx->d_kpmap, o.kp_scoremap ? (c.dev ? o.kp_scoremap : s_kpmap) : nullptr, 256 * 256 * 21);
    plan.add(ctx->d_coord, o.coord3d ? (c.dev ? o.coord3d : s_coord) : nullptr, 63);
    plan.add(ctx->d_kpcrop, o.kp_crop ? (c.dev ? (float*)o.kp_crop : s_kpcrop) : nullptr, 42);
    plan.add(ctx->d_kpimg, o.kp_image ? (c.dev ? (float*)o.kp_image : s_kpimg) : nullptr, 84);
    if (plan.n > 0) {
        ProfScope ps(ctx, "slot_scatter", "slot_scatter", 0.0, plan.bytes(ns, m));
        slot_scatter_launch(plan, d_pos, ns, ctx->stream);
    }
    HIPCHK(ctx, hipGetLastError());
    if (!c.dev) {
        CHK(copy_out(ctx, o.image_crop, s_crop, (size_t)ns * 256 * 256 * 3, false));
        CHK(copy_out(ctx, o.kp_scoremap, s_kpmap, (size_t)ns * 256 * 256 * 21, false));
        CHK(copy_out(ctx, o.coord3d, s_coord, (size_t)ns * 63, false));
        CHK(copy_out(ctx, (float*)o.kp_crop, s_kpcrop, (size_t)ns * 42, false));           // (int32 / float64: four bytes a word, as copy_out counts)
        CHK(copy_out(ctx, (float*)o.kp_image, s_kpimg, (size_t)ns * 84, false));
    }
    return 0;
}

// Up to K hands per frame: HandSegNet, the soft-max and ONE multi-hand mask growth per chunk of frames, then the back
// half of infer_full_impl -- PoseNet2D, the lifting towers with the heat-map up-sampling and the keypoint detection beside them -- at
// batch nb * K with per-slot centre / scale / hand_side.  No compaction unless option "hands_compact" (DESIGN.md 4.15): absent slots run on their fall-back crop, so a call has one
// kernel plan and no host wait.  A chunk holds at most micro_batch / K frames: no launch behind the crop sees more slots than a
// single-hand call's chunk has images.  One stream, no graph replay.
// (in.image_u8: host frames of Hin x Win, resized to the network's size; out.valid / out.area: per slot)
int infer_hands_impl(hp3d_ctx* ctx, int B, int H, int W, int K, const StepIn& in, int Hin, int Win, const StepOut& out, float* hand_scoremap,
                     float* hand_mask) {
    if (!ctx) return HP3D_ERR_ARG;
    const unsigned char* image_u8 = in.image_u8;
    const bool dev = in.dev;
    if ((!in.image && !image_u8) || !in.hand_side) HP3D_FAIL(ctx, HP3D_ERR_ARG, "image / hand_side is NULL");
    if (K < 1 || K > HP3D_MAX_HANDS) HP3D_FAIL(ctx, HP3D_ERR_ARG, "max hands K=%d must be in 1 ... %d", K, HP3D_MAX_HANDS);
    if (image_u8 && (Hin < 2 || Win < 2)) HP3D_FAIL(ctx, HP3D_ERR_ARG, "bad uint8 frame size %dx%d", Hin, Win);
    CHK(check_img(ctx, B, H, W));
    CHK(need_nets(ctx, NET_SEG | NET_POSE | NET_PRIOR | NET_VP));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int mb = slot_micro_batch(ctx, B, K, H, W);
    CHK(ensure_arena(ctx, mb, H, W, mb * K));
    if (hand_mask && (size_t)mb * K * H * W > ctx->mask_floats) {
        CHK(dev_realloc(ctx, &ctx->d_mask, (size_t)mb * K * H * W));
        ctx->mask_floats = (size_t)mb * K * H * W;
    }
    ProfCall prof(ctx);
    for (int b0 = 0; b0 < B; b0 += mb) {
        const int nb = std::min(mb, B - b0), ns = nb * K;
        const size_t s0 = (size_t)b0 * K;
        prof.chunk(b0);
        const float* d_img = in.image ? in.image + (size_t)b0 * H * W * 3 : nullptr;
        const float* d_hs = in.hand_side + s0 * 2;
        if (image_u8) {
            const size_t nbytes = (size_t)nb * Hin * Win * 3;
            if (nbytes > ctx->u8_bytes) { CHK(dev_realloc(ctx, &ctx->d_u8, nbytes)); ctx->u8_bytes = nbytes; }
            HIPCHK(ctx, hipMemcpyAsync(ctx->d_u8, image_u8 + (size_t)b0 * Hin * Win * 3, nbytes, hipMemcpyHostToDevice, ctx->stream));
            preprocess_u8_launch(ctx->d_u8, nb, Hin, Win, H, W, ctx->d_image, ctx->stream);
            d_img = ctx->d_image;
        } else if (!dev) {
            CHK(copy_in(ctx, ctx->d_image, d_img, (size_t)nb * H * W * 3, false));
            d_img = ctx->d_image;
        }
        if (!dev) { CHK(copy_in(ctx, ctx->d_hs, d_hs, (size_t)ns * 2, false)); d_hs = ctx->d_hs; }
        const StepOut o = out.at(s0);
        const bool want_kp = o.kp_crop || o.kp_image;
        FrameSrc src;
        src.f32 = d_img;
        CHK(run_detect_and_crop(ctx, d_img, nb, H, W, hand_mask != nullptr, image_u8 != nullptr, false, K));
        bool compacted = false;          // option "hands_compact": the back half ran on the valid slots only and wrote its outputs
        if (ctx->hands_compact) {
            CompactChunk cc{nb, K, H, W, nullptr, src, ctx->d_center, ctx->d_scale, d_hs, o, dev, want_kp};
            CHK(compact_wait_flags(ctx, ctx->d_valid, ns, &cc.h_valid));
            CHK(run_compact_back_half(ctx, cc, &compacted));
        }
        if (!compacted) {
            CHK(crop_frames(ctx, src, nb, K, H, W, ctx->d_center, ctx->d_scale));
            CHK(run_back_half(ctx, back_half_to(ctx, o, ns, d_hs, nullptr, nullptr, dev, want_kp), [] { return 0; }));
        }
        CHK(copy_out(ctx, hand_scoremap ? hand_scoremap + (size_t)b0 * H * W * 2 : nullptr, ctx->d_large, (size_t)nb * H * W * 2, dev));
        CHK(copy_out_slots(ctx, o, ns, ctx->d_scale, ctx->d_center, dev, !compacted));
        CHK(copy_out(ctx, hand_mask ? hand_mask + s0 * H * W : nullptr, ctx->d_mask, (size_t)ns * H * W, dev));
        CHK(copy_out(ctx, o.valid, ctx->d_valid, (size_t)ns, dev));
        CHK(copy_out(ctx, o.area, ctx->d_area, (size_t)ns, dev));
    }
    if (!dev) return finish_op(ctx);
    return 0;
}

// ---- tracking several hands per frame --------------------------------------------------------------------
int ensure_track_hands(hp3d_ctx* ctx, int n) {
    TrackHandsState& T = ctx->track_hands;
    if (n <= T.cap) return 0;
    CHK(T.h_flags.wait(ctx));
    for (int i = 0; i < 2; ++i) {
        CHK(dev_realloc(ctx, &T.center[i], (size_t)n * 2));
        CHK(dev_realloc(ctx, &T.scale[i], (size_t)n));
    }
    CHK(dev_realloc(ctx, &T.conf, (size_t)n));
    CHK(dev_realloc(ctx, &T.flags, (size_t)n * 2));
    CHK(dev_realloc(ctx, &T.detected, (size_t)n));
    CHK(dev_realloc(ctx, &T.area, (size_t)n));
    CHK(dev_realloc(ctx, &T.claimed, (size_t)n));
    CHK(dev_realloc(ctx, &T.keep, (size_t)n));
    CHK(T.h_flags.resize(ctx, (size_t)n * 2, "multi-hand tracking state"));
    T.cap = n;
    T.ok = false;
    return 0;
}

// the buffers of option "track_hands_partial_detect" for n slots: only a step that can be partial asks for them
int ensure_track_hands_partial(hp3d_ctx* ctx, int n) {
    TrackHandsState& T = ctx->track_hands;
    if (n <= T.pcap) return 0;
    CHK(dev_realloc(ctx, &T.pidx, (size_t)n));
    CHK(dev_realloc(ctx, &T.ppos, (size_t)n));
    CHK(dev_realloc(ctx, &T.keep_d, (size_t)n));
    CHK(dev_realloc(ctx, &T.claimed_d, (size_t)n));
    CHK(dev_realloc(ctx, &T.center_d, (size_t)n * 2));
    CHK(dev_realloc(ctx, &T.scale_d, (size_t)n));
    T.pcap = n;
    return 0;
}

void track_hands_free(hp3d_ctx* ctx) {
    TrackHandsState& T = ctx->track_hands;
    for (int i = 0; i < 2; ++i) {
        if (T.center[i]) hipFree(T.center[i]);
        if (T.scale[i]) hipFree(T.scale[i]);
    }
    for (void* p : {(void*)T.conf, (void*)T.flags, (void*)T.detected, (void*)T.area, (void*)T.claimed, (void*)T.keep, (void*)T.pidx, (void*)T.ppos,
                    (void*)T.keep_d, (void*)T.claimed_d, (void*)T.center_d, (void*)T.scale_d})
        if (p) hipFree(p);
    T.h_flags.free();
    T = TrackHandsState();
}

// One video step with K slots per frame.  A slot follows its hand for as long as it is not lost: the slot index is the hand's identity.
// DETECT step: HandSegNet once, the soft-max with fg, one claimed multi-hand growth per chunk (slots that are valid and not lost are
// kept: an object one of them claims is dropped, the others fill the free slots in the order of discovery), the per-slot select, then
// the crop.  TRACKED step: the K crops of a frame come from the state's boxes.  Behind the crop both are infer_hands_impl's back half
// at batch nb * K plus the per-slot box rule.  Decided on the host, before anything is enqueued, from the valid | lost flags that travel
// behind the previous step; the whole batch detects together; absent slots run on their fall-back crop (no compaction unless option
// "hands_compact", DESIGN.md 4.15: run_compact_back_half).  Option "track_hands_partial_detect" (DESIGN.md 4.18): a detect step that
// flags alone caused runs HandSegNet, the soft-max and the claimed growth per chunk at batch m = the chunk's frames with a valid slot lost
// or no valid slot, on those frames (0 < m < nb: "partial"; m = 0: the chunk is enqueued as a tracked chunk; m = nb: as without it).
int track_hands_step_impl(hp3d_ctx* ctx, int B, int H, int W, int K, const StepIn& in, const StepOut& out) {
    if ((!in.image && !in.raw()) || !in.hand_side) HP3D_FAIL(ctx, HP3D_ERR_ARG, "image / hand_side is NULL");
    if (K < 1 || K > HP3D_MAX_HANDS) HP3D_FAIL(ctx, HP3D_ERR_ARG, "max hands K=%d must be in 1 ... %d", K, HP3D_MAX_HANDS);
    if (in.nv) CHK(check_nv12(ctx, B, H, W, *in.nv));
    if (in.px) CHK(check_px(ctx, B, H, W, *in.px));
    if (in.surf) CHK(check_surfaces(ctx, B, H, W, in.surf));
    CHK(check_img(ctx, B, H, W));
    const bool dev = in.dev;
    int Hd, Wd;
    CHK(detect_frame(ctx, H, W, &Hd, &Wd));
    const int f = ctx->detect_scale;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    TrackHandsState& T = ctx->track_hands;
    CHK(T.h_flags.wait(ctx));                            // the only wait tracking adds: the previous step's flags
    const int n = B * K;
    const bool fresh = !T.ok || T.B != B || T.K != K || T.H != H || T.W != W || T.f != f;
    bool any_lost = false, no_hand = false;      // a valid slot was lost / an image has nothing to follow
    if (!fresh)
        for (int b = 0; b < B; ++b) {
            bool any_valid = false;
            for (int j = 0; j < K; ++j) {
                const bool v = T.h_flags.h[b * K + j] != 0;
                any_valid = any_valid || v;
                any_lost = any_lost || (v && T.h_flags.h[n + b * K + j] != 0);
            }
            no_hand = no_hand || !any_valid;
        }
    const bool sched = ctx->track_redetect > 0 && T.since + 1 >= ctx->track_redetect;
    const bool detect = fresh || any_lost || no_hand || sched;
    CHK(need_nets(ctx, (detect ? NET_SEG : 0) | NET_POSE | NET_PRIOR | NET_VP));
    const int mb = slot_micro_batch(ctx, B, K, Hd, Wd);
    CHK(ensure_arena(ctx, mb, Hd, Wd, mb * K));
    // option "track_hands_partial_detect": only a detect step that flags alone caused (a fresh one has nothing to keep, a scheduled one
    // is how a hand that enters any picture is found: both run whole)
    const bool partial_step = ctx->track_hands_partial_detect && detect && !fresh && !sched;
    // a host float32 frame is staged where the detection frame (f > 1) or the gathered frames (a partial chunk) go to d_image
    if ((f > 1 || partial_step) && !dev && !in.raw()) CHK(ensure_stage(ctx, (size_t)mb * H * W * 3));
    CHK(ensure_track_hands(ctx, n));
    if (partial_step) CHK(ensure_track_hands_partial(ctx, n));
    T.ok = false;                                        // a step that fails half way leaves no state behind
    T.B = B; T.K = K; T.H = H; T.W = W; T.f = f;         // (the flags' layout: lost() = flags + B K)
    if (fresh) HIPCHK(ctx, hipMemsetAsync(T.keep, 0, sizeof(int) * (size_t)n, ctx->stream));      // nothing to keep
    StepFrames fr{in, H, W};
    CHK(fr.upload(ctx, B));
    ProfCall prof(ctx);
    const int cur = T.cur, nxt = T.cur ^ 1;
    for (int b0 = 0; b0 < B; b0 += mb) {
        const int nb = std::min(mb, B - b0), ns = nb * K;
        const size_t s0 = (size_t)b0 * K;
        prof.chunk(b0);
        int m = nb;                                      // the chunk's frames that detect
        if (partial_step) {
            m = 0;
            for (int b = b0; b < b0 + nb; ++b) {
                bool any_valid = false, lost = false;
                for (int j = 0; j < K; ++j) {
                    const bool v = T.h_flags.h[b * K + j] != 0;
                    any_valid = any_valid || v;
                    lost = lost || (v && T.h_flags.h[n + b * K + j] != 0);
                }
                m += (lost || !any_valid) ? 1 : 0;
            }
        }
        const bool partial = partial_step && m > 0 && m < nb;
        const bool chunk_detect = detect && m > 0;       // (m = 0: another chunk holds the loss; this one runs as a tracked chunk)
        CHK(fr.chunk(ctx, b0, nb, K, f > 1 || partial));
        FrameSrc crop_src = fr.src;
        float* bc = T.center[cur] + s0 * 2;
        float* bs = T.scale[cur] + s0;
        if (partial) {           // idx / pos from the flags, which this chunk's select and box rule have not overwritten yet
            int* pidx = T.pidx + b0;
            int* ppos = T.ppos + b0;
            {
                ProfScope ps(ctx, "track_hands_partial_index", "track_hands_partial_index", 0.0, 8.0 * ns + 8.0 * nb);
                track_hands_partial_index_launch(T.valid() + s0, T.lost() + s0, nb, K, pidx, ppos, ctx->stream);
            }
            ctx->track_hands_partial_frames_run += m;
            ctx->track_hands_partial_frames_skipped += nb - m;
            MaskKeep mk;         // keep and the boxes of the m * K slots, dense: what the claimed growth at batch m reads
            mk.keep = T.keep_d; mk.center = T.center_d; mk.scale = T.scale_d; mk.claimed = T.claimed_d;
            {
                ProfScope ps(ctx, "track_hands_slot_gather", "track_hands_slot_gather", 0.0, 32.0 * m * K);
                track_hands_slot_gather_launch(pidx, m, K, T.keep + s0, bc, bs, T.keep_d, T.center_d, T.scale_d, ctx->stream);
            }
            // the m frames, dense, into d_image: never the buffer the chunk's frames lie in (a host frame was staged in d_stage)
            if (f > 1) {
                CHK(run_detect_reduced(ctx, fr.src, m, H, W, Hd, Wd, K, mk, pidx));
            } else {
                if (in.raw()) {
                    CHK(normalise_frames(ctx, fr.src, pidx, m, H, W));
                } else {
                    ProfScope ps(ctx, "frame_gather", "frame_gather", 0.0, 8.0 * m * H * W * 3);
                    frame_gather_launch(fr.src.f32, pidx, m, (size_t)H * W * 3, ctx->d_image, ctx->stream);
                    ++ctx->frame_gather_launches;
                }
                HIPCHK(ctx, hipGetLastError());
                CHK(run_detect_and_crop(ctx, ctx->d_image, m, H, W, 0, true, false, K, mk));
            }
            ProfScope ps(ctx, "track_hands_select_pos", "track_hands_select_pos", 0.0, 4.0 * nb + 44.0 * ns);
            track_hands_select_pos_launch(ppos, nb, K, T.keep + s0, ctx->d_center, ctx->d_scale, ctx->d_valid, ctx->d_area, T.claimed_d, bc, bs,
                                          T.valid() + s0, T.detected + s0, T.area + s0, T.claimed + s0, ctx->stream);
            // (a raw frame: all nb * K crops straight from it = normalise, then crop, bit for bit)
        } else if (chunk_detect) {
            MaskKeep mk;
            mk.keep = T.keep + s0; mk.center = bc; mk.scale = bs; mk.claimed = T.claimed + s0;
            CHK(run_detect_front(ctx, fr.src, nb, H, W, Hd, Wd, K, mk, &crop_src));
            ProfScope ps(ctx, "track_hands_select", "track_hands_select", 0.0, 40.0 * ns);
            track_hands_select_launch(T.keep + s0, ctx->d_center, ctx->d_scale, ctx->d_valid, ctx->d_area, ns, bc, bs, T.valid() + s0,
                                      T.detected + s0, T.area + s0, ctx->stream);
        }
        HIPCHK(ctx, hipGetLastError());
        const StepOut o = out.at(s0);
        // the state a tracked step's box rule also clears (a detect step's select has written it)
        int* detected0 = chunk_detect ? nullptr : T.detected + s0;
        int* area0 = chunk_detect ? nullptr : T.area + s0;
        int* claimed0 = chunk_detect ? nullptr : T.claimed + s0;
        bool compacted = false;          // option "hands_compact": the back half ran on the valid slots only and wrote its outputs
        if (ctx->hands_compact) {
            const std::function<void(const double*, const int*)> box = [&](const double* kp_dense, const int* d_pos) {
                ProfScope ps(ctx, "track_hands_box", "track_hands_box_pos", 0.0, 4.0 * ns * 32 * 32 * 21);
                track_hands_box_pos_launch(kp_dense, ctx->d_sm[2], 32, ns, H, W, 256, ctx->track_margin, ctx->track_min_score,
                                           ctx->track_use_min_score, d_pos, bc, bs, T.center[nxt] + s0 * 2, T.scale[nxt] + s0, T.conf + s0,
                                           T.lost() + s0, T.keep + s0, detected0, area0, claimed0, ctx->stream);
            };
            // (a tracked step: the state's flags are on the host already)
            CompactChunk cc{nb, K, H, W, T.h_flags.h + s0, crop_src, bc, bs, fr.d_hs, o, dev, true, &box};
            if (chunk_detect) CHK(compact_wait_flags(ctx, T.valid() + s0, ns, &cc.h_valid));
            CHK(run_compact_back_half(ctx, cc, &compacted));
        }
        if (!compacted) {
            CHK(crop_frames(ctx, crop_src, nb, K, H, W, bc, bs));
            CHK(run_back_half(ctx, back_half_to(ctx, o, ns, fr.d_hs, bc, bs, dev, true), [&]() -> int {
                ProfScope ps(ctx, "track_hands_box", "track_hands_box", 0.0, 4.0 * ns * 32 * 32 * 21);
                track_hands_box_launch(dev && o.kp_image ? o.kp_image : ctx->d_kpimg, ctx->d_sm[2], 32, ns, H, W, 256, ctx->track_margin,
                                       ctx->track_min_score, ctx->track_use_min_score, T.valid() + s0, bc, bs, T.center[nxt] + s0 * 2,
                                       T.scale[nxt] + s0, T.conf + s0, T.lost() + s0, T.keep + s0, detected0, area0, claimed0, ctx->stream);
                return 0;
            }));
        }
        CHK(copy_out_slots(ctx, o, ns, bs, bc, dev, !compacted));
        CHK(copy_out(ctx, o.confidence, T.conf + s0, (size_t)ns, dev));
        CHK(copy_out(ctx, o.lost, T.lost() + s0, (size_t)ns, dev));
        CHK(copy_out(ctx, o.detected, T.detected + s0, (size_t)ns, dev));
        CHK(copy_out(ctx, o.valid, T.valid() + s0, (size_t)ns, dev));
        CHK(copy_out(ctx, o.area, T.area + s0, (size_t)ns, dev));
        CHK(copy_out(ctx, o.claimed, T.claimed + s0, (size_t)ns, dev));
    }
    CHK(T.h_flags.copy_behind(ctx, T.flags, (size_t)n * 2));
    T.cur = nxt; T.ok = true;
    T.since = detect ? 0 : T.since + 1;
    ++(detect ? ctx->track_hands_detect_steps : ctx->track_hands_tracked_steps);
    if (detect && f > 1) ++ctx->detect_scale_steps;
    if (!dev) return finish_op(ctx);
    return 0;
}

}  // namespace

// ================================================================================================
// hp3d_set_option("graph", "1"): the device-pointer entry points replay their whole launch sequence (~85 launches for
// the full path) as one hipGraph once the same call (shape + pointers) is seen for the third time: call 1 runs normally
// (allocations, function attributes), call 2 is captured while it is enqueued, later calls are a single
// hipGraphLaunch.  Anything the sequence depends on (arena re-allocation, weights, options, profiling) bumps
// graph_epoch and drops the captured graphs.  Meant for small batches, where launch gaps are ~15 % of the time.
template <class F>
int run_graphed(hp3d_ctx* ctx, const std::string& key, F&& enqueue) {
#ifdef HP3D_EMU
    return enqueue();
#else
    if (!ctx->use_graph || ctx->profiling) return enqueue();
    hp3d_ctx::GraphEntry& g = ctx->graphs[key];
    if (g.exec && g.epoch != ctx->graph_epoch) { hipGraphExecDestroy(g.exec); g.exec = nullptr; g.calls = 0; }
    if (g.exec) {
        HIPCHK(ctx, hipGraphLaunch(g.exec, ctx->stream));
        ++ctx->graph_replays;
        return 0;
    }
    if (g.calls < 0 || g.calls++ == 0) return enqueue();                  // warm-up (or capture failed earlier)
    const long epoch0 = ctx->graph_epoch;
    if (hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) { g.calls = -1; return enqueue(); }
    const int rc = enqueue();
    hipGraph_t graph = nullptr;
    const hipError_t e = hipStreamEndCapture(ctx->stream, &graph);
    if (rc != 0 || e != hipSuccess || !graph || epoch0 != ctx->graph_epoch) {          // not capturable: stay on plain launches
        if (getenv("HP3D_GRAPH_DEBUG")) fprintf(stderr, "hp3d graph: capture of %s failed (rc %d, %s, epoch %ld -> %ld)\n", key.c_str(), rc, hipGetErrorString(e), epoch0, ctx->graph_epoch);
        if (graph) hipGraphDestroy(graph);
        (void)hipGetLastError();
        g.calls = -1;
        return rc != 0 ? rc : enqueue();
    }
    const hipError_t ei = hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0);
    hipGraphDestroy(graph);
    if (ei != hipSuccess) { g.exec = nullptr; g.calls = -1; (void)hipGetLastError(); return enqueue(); }
    g.epoch = ctx->graph_epoch;
    if (getenv("HP3D_GRAPH_DEBUG")) fprintf(stderr, "hp3d graph: captured %s\n", key.c_str());
    ++ctx->graph_captures;
    HIPCHK(ctx, hipGraphLaunch(g.exec, ctx->stream));
    ++ctx->graph_replays;
    return 0;
#endif
}
static std::string graph_key(const char* what, std::initializer_list<long> dims, std::initializer_list<const void*> ptrs) {
    char buf[64];
    std::string k(what);
    for (long d : dims) { snprintf(buf, sizeof buf, "|%ld", d); k += buf; }
    for (const void* p : ptrs) { snprintf(buf, sizeof buf, "|%p", p); k += buf; }
    return k;
}

static long long comm_ranks(hp3d_ctx* ctx);     // ranks of the live RCCL communicator (ncclCommCount), 0 = none

extern "C" {

int hp3d_abi_version(void) { return 1; }

int hp3d_device_count(int* count) {
    if (!count) return HP3D_ERR_ARG;
    *count = 0;
#ifdef HP3D_EMU
    *count = 1;             // the CPU interpreter plays one device
    return 0;
#else
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return HP3D_ERR_HIP; }
    *count = n;
    return 0;
#endif
}

int hp3d_device_pci_bus_id(int device, char* buf, int cap) {
    if (!buf || cap < 13) return HP3D_ERR_ARG;
    buf[0] = 0;
#ifdef HP3D_EMU
    (void)device;
    return HP3D_ERR_UNSUPPORTED;          // the CPU interpreter's one device sits on no bus
#else
    if (hipDeviceGetPCIBusId(buf, cap, device) != hipSuccess) { (void)hipGetLastError(); buf[0] = 0; return HP3D_ERR_HIP; }
    return 0;
#endif
}

int hp3d_create(int device, hp3d_ctx** out) {
    if (!out) return HP3D_ERR_ARG;
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        set_error(nullptr, "hp3d_create: no HIP device visible (the engine has no CPU fallback)");
        return HP3D_ERR_HIP;
    }
    if (device < 0 || device >= n) {
        set_error(nullptr, "hp3d_create: device index out of range");
        return HP3D_ERR_ARG;
    }
    hp3d_ctx* ctx = new hp3d_ctx();
    ctx->device = device;
    ctx->use_wino4 = wino4_default();
    if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&ctx->stream) != hipSuccess) {
        set_error(nullptr, "hp3d_create: hipSetDevice/hipStreamCreate failed");
        delete ctx;
        return HP3D_ERR_HIP;
    }
    *out = ctx;
    return 0;
}

int hp3d_destroy(hp3d_ctx* ctx) {
    if (!ctx) return HP3D_ERR_ARG;
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
#ifndef HP3D_EMU
    if (ctx->copy_stream) hipStreamSynchronize(ctx->copy_stream);
#endif
    if (ctx->kid) { hp3d_destroy(ctx->kid); ctx->kid = nullptr; }
#ifndef HP3D_EMU
    if (ctx->ev_fork) hipEventDestroy(ctx->ev_fork);
    if (ctx->ev_join) hipEventDestroy(ctx->ev_join);
#endif
    if (ctx->shared_weights) { ctx->blob = nullptr; ctx->blob16 = nullptr; }     // owned by the parent context
    float** fp[] = {&ctx->blob, &ctx->bufA, &ctx->bufB, &ctx->col, &ctx->d_image, &ctx->d_hs, &ctx->d_large,
                    &ctx->d_crop, &ctx->d_center, &ctx->d_scale, &ctx->d_cropsize, &ctx->d_kpmap, &ctx->d_coord,
                    &ctx->d_mask, &ctx->d_segsmall, &ctx->d_concat, &ctx->d_sm[0], &ctx->d_sm[1], &ctx->d_sm[2],
                    &ctx->d_can, &ctx->d_rot, &ctx->d_u, &ctx->d_fc1, &ctx->d_fc2, &ctx->d_fg,
                    &ctx->d_pooled, &ctx->d_fcpart, &ctx->d_stage, &ctx->d_keepc, &ctx->d_keeps};
    for (float** p : fp)
        if (*p) hipFree(*p);
    if (ctx->d_kpimg) hipFree(ctx->d_kpimg);
    if (ctx->d_gather) hipFree(ctx->d_gather);
#ifndef HP3D_EMU
    if (ctx->upload_done) hipEventDestroy(ctx->upload_done);
    if (ctx->copy_stream) hipStreamDestroy(ctx->copy_stream);
#endif
    if (ctx->d_kpcrop) hipFree(ctx->d_kpcrop);
#ifndef HP3D_EMU
    for (auto& kv : ctx->graphs)
        if (kv.second.exec) hipGraphExecDestroy(kv.second.exec);
#endif
    if (ctx->comm) hp3d_comm_destroy(ctx);
    if (ctx->d_seed) hipFree(ctx->d_seed);
    if (ctx->d_valid) hipFree(ctx->d_valid);
    if (ctx->d_area) hipFree(ctx->d_area);
    if (ctx->d_liftbar) hipFree(ctx->d_liftbar);
#ifndef HP3D_EMU
    if (ctx->h_lifterr) hipHostFree(ctx->h_lifterr);
#endif
    if (ctx->d_keys) hipFree(ctx->d_keys);
    if (ctx->d_det) hipFree(ctx->d_det);
    if (ctx->d_mgscratch) hipFree(ctx->d_mgscratch);
    track_free(ctx);
    track_hands_free(ctx);
    compact_free(ctx);
    surf_free(ctx);
    if (ctx->d_u8) hipFree(ctx->d_u8);
    if (ctx->blob16) hipFree(ctx->blob16);
    if (ctx->d_concat16) hipFree(ctx->d_concat16);
    for (auto& kv : ctx->naive_w) hipFree(kv.second);
    for (hipEvent_t e : ctx->event_pool) hipEventDestroy(e);
    hipStreamDestroy(ctx->stream);
    delete ctx;
    return 0;
}

const char* hp3d_last_error(hp3d_ctx* ctx) { return ctx ? ctx->err.c_str() : g_last_error.c_str(); }
void* hp3d_stream(hp3d_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }
int hp3d_sync(hp3d_ctx* ctx) {
    if (!ctx) return HP3D_ERR_ARG;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return check_lift_error(ctx);
}

// ---- device / pinned-host memory for callers that hold their batches in HBM (bench.py, dist.py): the C ABI needs no
//      PyTorch for that.  Copies are ordered on the engine stream (hp3d_memcpy blocks until done); hp3d_upload_async
//      runs on a second stream so that the H2D of batch n+1 overlaps the kernels of batch n, hp3d_wait_upload makes
//      the engine stream wait for the last upload.
int hp3d_dev_alloc(hp3d_ctx* ctx, size_t bytes, void** out) {
    if (!ctx || !out) return HP3D_ERR_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    void* p = nullptr;
    if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) { (void)hipGetLastError(); HP3D_FAIL(ctx, HP3D_ERR_NOMEM, "hipMalloc(%zu) failed", bytes); }
    *out = p;
    return 0;
}
int hp3d_dev_free(hp3d_ctx* ctx, void* p) {
    if (!ctx) return HP3D_ERR_ARG;
    if (!p) return 0;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->copy_stream) HIPCHK(ctx, hipStreamSynchronize(ctx->copy_stream));    // a pending hp3d_upload_async may target it
    if (ctx->kid) HIPCHK(ctx, hipStreamSynchronize(ctx->kid->stream));
    HIPCHK(ctx, hipFree(p));
    return 0;
}
#ifndef HP3D_EMU
int hp3d_host_alloc(hp3d_ctx* ctx, size_t bytes, void** out) {
    if (!ctx || !out) return HP3D_ERR_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); HP3D_FAIL(ctx, HP3D_ERR_NOMEM, "hipHostMalloc(%zu) failed", bytes); }
    *out = p;
    return 0;
}
int hp3d_host_free(hp3d_ctx* ctx, void* p) {
    if (!ctx) return HP3D_ERR_ARG;
    if (!p) return 0;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (ctx->copy_stream) HIPCHK(ctx, hipStreamSynchronize(ctx->copy_stream));    // an upload may still be reading the buffer
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipHostFree(p));
    return 0;
}
int hp3d_upload_async(hp3d_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes) {
    if (!ctx || !dst_dev || !src_host) return HP3D_ERR_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (!ctx->copy_stream) {
        HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
        HIPCHK(ctx, hipEventCreateWithFlags(&ctx->upload_done, hipEventDisableTiming));
    }
    HIPCHK(ctx, hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, ctx->copy_stream));
    HIPCHK(ctx, hipEventRecord(ctx->upload_done, ctx->copy_stream));
    return 0;
}
int hp3d_wait_upload(hp3d_ctx* ctx) {
    if (!ctx) return HP3D_ERR_ARG;
    if (ctx->upload_done) HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->upload_done, 0));
    return 0;
}
#else
int hp3d_host_alloc(hp3d_ctx* ctx, size_t bytes, void** out) { if (!ctx || !out) return HP3D_ERR_ARG; *out = malloc(bytes ? bytes : 1); return *out ? 0 : HP3D_ERR_NOMEM; }
int hp3d_host_free(hp3d_ctx* ctx, void* p) { if (!ctx) return HP3D_ERR_ARG; free(p); return 0; }
int hp3d_upload_async(hp3d_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes) {
    if (!ctx || !dst_dev || !src_host) return HP3D_ERR_ARG;
    memcpy(dst_dev, src_host, bytes);
    return 0;
}
int hp3d_wait_upload(hp3d_ctx* ctx) { return ctx ? 0 : HP3D_ERR_ARG; }
#endif
int hp3d_memcpy(hp3d_ctx* ctx, void* dst, const void* src, size_t bytes, int kind) {
    if (!ctx || !dst || !src || kind < 0 || kind > 2) return HP3D_ERR_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const hipMemcpyKind k = kind == 0 ? hipMemcpyHostToDevice : kind == 1 ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    HIPCHK(ctx, hipMemcpyAsync(dst, src, bytes, k, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

int hp3d_set_option(hp3d_ctx* ctx, const char* key, const char* value) {
    if (!ctx || !key || !value) return HP3D_ERR_ARG;
    const std::string k(key), v(value);
    ++ctx->graph_epoch;             // captured launch sequences may depend on any option
    if (k == "empty_reduce" && (v == "inf" || v == "fltmax")) { ctx->empty_fltmax = (v == "fltmax"); return 0; }
    if (k == "wino_splitk" && (v == "0" || v == "1")) { ctx->wino_splitk = v == "1"; return 0; }
    if (k == "wino4_tail" && (v == "0" || v == "1")) { ctx->w4_tail = v == "1"; ++ctx->graph_epoch; return 0; }
    if (k == "first_touch_beside" && (v == "0" || v == "1")) { ctx->first_touch_beside = v == "1"; return 0; }
    if (k == "first_touch" && (v == "0" || v == "1" || v == "auto")) { ctx->first_touch = v == "auto" ? -1 : v == "1"; return 0; }
    if (k == "first_walk" && (v == "balanced" || v == "rows")) { ctx->first_balanced = v == "balanced"; return 0; }
    if (k == "lift_overlap" && (v == "0" || v == "1")) { ctx->lift_overlap = v == "1"; return 0; }
    if (k == "lift_fused" && (v == "0" || v == "1" || v == "auto")) { ctx->use_lift_fused = v == "auto" ? -1 : v == "1" ? 1 : 0; return 0; }
    if (k == "wino4" && (v == "0" || v == "1" || v == "pose" || v == "auto" || v == "all")) {
        ctx->use_wino4 = v == "auto" ? wino4_default() : v == "all" ? -2 : v == "1" ? 1 : v == "pose" ? -1 : 0;
        return 0;
    }
    if (k == "wino4_split" && (v == "0" || v == "1" || v == "auto")) { ctx->use_wino4s = v == "auto" ? -1 : v == "1" ? 1 : 0; return 0; }
    if (k == "fc_tail" && (v == "0" || v == "1")) { ctx->fc_tail = v == "1"; return 0; }
    if (k == "kp_up_side" && (v == "0" || v == "1")) { ctx->kp_up_side = v == "1"; return 0; }
    if (k == "tiny_gemm" && (v == "0" || v == "1")) { ctx->tiny_gemm = v == "1"; return 0; }
    if (k == "pw2" && (v == "0" || v == "1" || v == "force")) { ctx->use_pw2 = v == "0" ? 0 : v == "1" ? 1 : 2; return 0; }
    if (k == "wino7_ksplit") { ctx->wino7_ksplit = v == "auto" ? 0 : std::max(0, atoi(v.c_str())); return 0; }
    if (k == "wino7" && (v == "0" || v == "1" || v == "auto")) { ctx->use_wino7 = v == "auto" ? -1 : v == "1" ? 1 : 0; return 0; }
    if (k == "wino2" && (v == "0" || v == "1" || v == "auto")) { ctx->use_wino2 = v == "auto" ? -1 : v == "1" ? 1 : 0; return 0; }
    if (k == "f16_fuse12" && (v == "0" || v == "1" || v == "ring" || v == "resident")) {
        ctx->fuse12 = v == "0" ? 0 : v == "1" ? 1 : v == "ring" ? 2 : 3; ++ctx->graph_epoch; return 0;
    }
    if (k == "f16_k7k1" && (v == "0" || v == "1")) { ctx->h16_k7k1 = v == "1"; return 0; }
    if (k == "f16_impl" && (v == "h16" || v == "mfma" || v == "h16_force")) { ctx->use_h16 = v == "mfma" ? 0 : v == "h16" ? 1 : 2; return 0; }
    if (k == "mask_grow" && (v == "auto" || v == "lds" || v == "global")) { ctx->mask_grow = v == "auto" ? 0 : v == "lds" ? 1 : 2; return 0; }
    if (k == "streams" && (v == "1" || v == "2" || v == "auto")) { ctx->nstreams = v == "auto" ? -1 : v == "2" ? 2 : 1; return 0; }
    if (k == "conv_impl" && (v == "mfma" || v == "naive" || v == "direct" || v == "winograd")) {
        ctx->conv_naive = (v == "naive");
        ctx->use_wino = (v == "direct" || v == "naive") ? 0 : (v == "winograd") ? 2 : 1;   // mfma = auto
        ctx->use_first = (v == "direct" || v == "naive") ? 0 : 1;
        return 0;
    }
    if (k == "graph" && (v == "0" || v == "1")) {
#ifdef HP3D_EMU
        if (v == "1") HP3D_FAIL(ctx, HP3D_ERR_UNSUPPORTED, "no hipGraph in the CPU interpreter build");
#endif
        ctx->use_graph = v == "1";
        return 0;
    }
    if (k == "track_margin" || k == "track_min_score") {
        if (k == "track_min_score" && v == "off") { ctx->track_use_min_score = 0; return 0; }
        char* end = nullptr;
        const float f = strtof(value, &end);
        if (end == value || *end || !(f == f) || (k == "track_margin" && !(f > 0.f && f <= 16.f)))
            HP3D_FAIL(ctx, HP3D_ERR_ARG, "%s wants a number%s, got %s", key, k == "track_margin" ? " in (0, 16]" : " or \"off\"", value);
        if (k == "track_margin") ctx->track_margin = f;
        else { ctx->track_min_score = f; ctx->track_use_min_score = 1; }
        return 0;
    }
    if (k == "hands_min_area") {
        char* end = nullptr;
        const long n = strtol(value, &end, 10);
        if (end == value || *end || n < 0 || n > (1L << 30)) HP3D_FAIL(ctx, HP3D_ERR_ARG, "hands_min_area wants a non-negative integer (0 = off), got %s", value);
        ctx->hands_min_area = (int)n;
        return 0;
    }
    if (k == "detect_scale") {
        if (v.size() != 1 || v[0] < '1' || v[0] > '8') HP3D_FAIL(ctx, HP3D_ERR_ARG, "detect_scale wants an integer in 1 ... 8, got %s", value);
        ctx->detect_scale = v[0] - '0';
        return 0;
    }
    if (k == "hands_compact") {
        if (v != "0" && v != "1") HP3D_FAIL(ctx, HP3D_ERR_ARG, "hands_compact wants 0 or 1, got %s", value);
        ctx->hands_compact = v == "1";
        return 0;
    }
    if (k == "track_hands_partial_detect") {
        if (v != "0" && v != "1") HP3D_FAIL(ctx, HP3D_ERR_ARG, "track_hands_partial_detect wants 0 or 1, got %s", value);
        ctx->track_hands_partial_detect = v == "1";
        return 0;
    }
    if (k == "track_partial_detect") {
        if (v != "0" && v != "1") HP3D_FAIL(ctx, HP3D_ERR_ARG, "track_partial_detect wants 0 or 1, got %s", value);
        ctx->track_partial_detect = v == "1";
        return 0;
    }
    if (k == "nv12_matrix") {
        const int m = nv12_matrix_index(value);
        if (m < 0) HP3D_FAIL(ctx, HP3D_ERR_ARG, "nv12_matrix wants bt709, bt601, bt709_full or bt601_full, got %s", value);
        ctx->nv12_matrix = m;
        return 0;
    }
    if (k == "track_redetect") {
        char* end = nullptr;
        const long n = strtol(value, &end, 10);
        if (end == value || *end || n < 0 || n > (1 << 20)) HP3D_FAIL(ctx, HP3D_ERR_ARG, "track_redetect wants a non-negative integer, got %s", value);
        ctx->track_redetect = (int)n;
        return 0;
    }
    if (k == "micro_batch" && v == "auto") { ctx->micro_batch = -1; return 0; }
    if (k == "micro_batch") {
        char* end = nullptr;
        const long n = strtol(value, &end, 10);
        if (end == value || *end || n < 0 || n > (1 << 20)) HP3D_FAIL(ctx, HP3D_ERR_ARG, "micro_batch wants a non-negative integer, got %s", value);
        ctx->micro_batch = (int)n;
        return 0;
    }
    HP3D_FAIL(ctx, HP3D_ERR_ARG, "unknown option %s=%s", key, value);
}

int hp3d_set_weight(hp3d_ctx* ctx, const char* tf_var_name, const float* data, const int64_t* shape, int rank) {
    if (!ctx || !tf_var_name || !data || !shape || rank < 1 || rank > 4) return HP3D_ERR_ARG;
    std::string name(tf_var_name);
    const size_t slash = name.rfind('/');
    if (slash == std::string::npos) HP3D_FAIL(ctx, HP3D_ERR_ARG, "bad variable name %s", tf_var_name);
    const std::string layer = name.substr(0, slash), kind = name.substr(slash + 1);
    if (kind != "weights" && kind != "biases") HP3D_FAIL(ctx, HP3D_ERR_ARG, "bad variable name %s", tf_var_name);
    std::vector<int64_t> want;
    bool known = false;
    auto ci = ctx->T.conv_idx.find(layer);
    if (ci != ctx->T.conv_idx.end()) {
        const ConvL& l = ctx->T.conv[ci->second];
        want = (kind == "weights") ? std::vector<int64_t>{l.k, l.k, l.cin, l.cout} : std::vector<int64_t>{l.cout};
        known = true;
    } else if (layer == "ViewpointNet/fc_vp_ux" || layer == "ViewpointNet/fc_vp_uy" || layer == "ViewpointNet/fc_vp_uz") {
        want = (kind == "weights") ? std::vector<int64_t>{128, 1} : std::vector<int64_t>{1};
        known = true;
    } else if (layer == "PosePrior/fc_xyz") {
        // [512,63] (proposed/direct) or [30,63] (bottleneck variant, nets/PosePriorNetwork.py:115-116)
        if (kind == "weights" && rank == 2 && shape[0] == 30) { want = {30, 63}; name = "PosePrior/fc_xyz#bn/weights"; }
        else want = (kind == "weights") ? std::vector<int64_t>{512, 63} : std::vector<int64_t>{63};
        known = true;
    } else {
        auto fi = ctx->T.fc_idx.find(layer);
        if (fi != ctx->T.fc_idx.end()) {
            const FcL& l = ctx->T.fc[fi->second];
            want = (kind == "weights") ? std::vector<int64_t>{l.cin, l.cout} : std::vector<int64_t>{l.cout};
            known = true;
        }
    }
    if (!known) HP3D_FAIL(ctx, HP3D_ERR_ARG, "unknown variable %s", tf_var_name);
    if ((int)want.size() != rank) HP3D_FAIL(ctx, HP3D_ERR_ARG, "rank mismatch for %s", tf_var_name);
    size_t n = 1;
    for (int i = 0; i < rank; ++i) {
        if (shape[i] != want[i]) HP3D_FAIL(ctx, HP3D_ERR_ARG, "shape mismatch for %s (dim %d: got %lld want %lld)",
                                           tf_var_name, i, (long long)shape[i], (long long)want[i]);
        n *= (size_t)shape[i];
    }
    HostVar v;
    v.data.assign(data, data + n);
    v.shape.assign(shape, shape + rank);
    ctx->vars[name] = std::move(v);
    return 0;
}

int hp3d_finalize_weights(hp3d_ctx* ctx, int dtype) {
    if (ctx) ++ctx->graph_epoch;
    if (!ctx) return HP3D_ERR_ARG;
    if (dtype != 0 && dtype != 1) HP3D_FAIL(ctx, HP3D_ERR_UNSUPPORTED, "dtype must be 0 (f32) or 1 (f16 trunks)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const bool pack_timing = getenv("HP3D_PACK_TIMING") != nullptr;      // diagnostics: host seconds of the phases below on stderr
    auto now = []() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    double t_mark = now();
    auto lap = [&](const char* what) {
        if (pack_timing) fprintf(stderr, "hp3d_finalize_weights: %-28s %.2f s\n", what, now() - t_mark);
        t_mark = now();
    };
    // staging: the packed blob is assembled on the host and uploaded once.  (The CPU interpreter's "device" memory IS host memory: it
    // packs straight into the blob -- copying 1.3 GB once more costs tens of seconds in the sandboxes the CPU suite runs in.)
#ifdef HP3D_EMU
    // (in place is safe against the one failure below, "incomplete variable set": variables can only be ADDED to a context, so every network
    //  that was complete before this call is complete now, and all packing is done before that check -- the blob then holds every complete
    //  network repacked in full, which is what ctx->nets still says)
    if (!ctx->blob) CHK(dev_realloc(ctx, &ctx->blob, ctx->T.blob_floats));
    memset(ctx->blob, 0, sizeof(float) * ctx->T.blob_floats);
    struct { float* p; float* data() { return p; } float& operator[](size_t i) { return p[i]; } } host{ctx->blob};
#else
    std::vector<float> host(ctx->T.blob_floats, 0.f);
#endif
    lap("blob allocation");
    int have = 0, partial = 0, bn_ok = 0;
    auto mark = [&](int net, bool present) {
        if (present) have |= net; else partial |= net;
    };
    // the convolution layers pack into disjoint regions of the blob: one task per layer, run on a few host threads (the 36-plane
    // F(4x4,3x3) copies made this 40 s on one thread)
    std::vector<std::function<void()>> pack_tasks;
    for (const ConvL& l : ctx->T.conv) {
        const HostVar *w = nullptr, *b = nullptr;
        const bool ok = find_var(ctx, l.name + "/weights", &w) == 0 && find_var(ctx, l.name + "/biases", &b) == 0;
        mark(l.net, ok);
        if (!ok) continue;
        const ConvL* lp = &l;
        float* hp = host.data();
        pack_tasks.push_back([lp, w, b, hp]() { pack_layer(*lp, w->data.data(), b->data.data(), hp); });
    }
    {
        std::atomic<size_t> next{0};
        auto worker = [&]() { for (size_t i; (i = next.fetch_add(1)) < pack_tasks.size();) pack_tasks[i](); };
        unsigned nthr = std::min<unsigned>(16, std::max(1u, std::thread::hardware_concurrency()));
        nthr = (unsigned)std::min<size_t>(nthr, pack_tasks.size());
        std::vector<std::thread> pool;
        for (unsigned t = 1; t < nthr; ++t) pool.emplace_back(worker);
        worker();
        for (auto& t : pool) t.join();
    }
    lap("conv layers (threads)");
    for (const FcL& l : ctx->T.fc) {
        if (l.name == "ViewpointNet/fc_vp_u") {
            const HostVar *w[3], *b[3];
            const char* ax[3] = {"ux", "uy", "uz"};
            bool ok = true;
            for (int a = 0; a < 3; ++a)
                ok = ok && find_var(ctx, std::string("ViewpointNet/fc_vp_") + ax[a] + "/weights", &w[a]) == 0 &&
                     find_var(ctx, std::string("ViewpointNet/fc_vp_") + ax[a] + "/biases", &b[a]) == 0;
            mark(l.net, ok);
            if (ok)
                for (int a = 0; a < 3; ++a) {
                    for (int i = 0; i < 128; ++i) host[l.w_off + (size_t)i * 3 + a] = w[a]->data[i];
                    host[l.b_off + a] = b[a]->data[0];
                }
            continue;
        }
        std::string bias_name = l.name + "/biases";
        if (l.name == "PosePrior/fc_xyz#bn") bias_name = "PosePrior/fc_xyz/biases";
        const HostVar *w = nullptr, *b = nullptr;
        const bool ok = find_var(ctx, l.name + "/weights", &w) == 0 && find_var(ctx, bias_name, &b) == 0;
        if (l.name == "PosePrior/fc_xyz") {
            // absent in the bottleneck variant: not an error there
            if (!ok && ctx->vars.count("PosePrior/fc_xyz#bn/weights")) continue;
        }
        if (l.net == NET_BOTTLENECK) { if (ok) ++bn_ok; }
        else mark(l.net, ok);
        if (ok) {
            memcpy(&host[l.w_off], w->data.data(), sizeof(float) * (size_t)l.cin * l.cout);
            memcpy(&host[l.b_off], b->data.data(), sizeof(float) * l.cout);
        }
    }
    const int bad = have & partial & (NET_SEG | NET_POSE | NET_PRIOR | NET_VP);
    if (bad) HP3D_FAIL(ctx, HP3D_ERR_WEIGHTS, "incomplete variable set for network mask %d", bad);
    lap("fc layers");
#ifndef HP3D_EMU
    if (!ctx->blob) CHK(dev_realloc(ctx, &ctx->blob, ctx->T.blob_floats));
    HIPCHK(ctx, hipMemcpy(ctx->blob, host.data(), sizeof(float) * ctx->T.blob_floats, hipMemcpyHostToDevice));
#endif
    lap("blob upload");
    ctx->nets = have & ~partial;
    if (bn_ok == 2) ctx->nets |= NET_BOTTLENECK;
    ctx->prec = dtype;
    if (dtype == 1) {    // half-precision copies of the HandSegNet / PoseNet2D filters (biases, heads' outputs and the lifting nets stay f32)
        std::vector<hp3d_f16> h16(ctx->T.blob16_halves, (hp3d_f16)0.f);
        for (const ConvL& l : ctx->T.conv) {
            if (!(l.net == NET_SEG || l.net == NET_POSE) || !(ctx->nets & l.net)) continue;
            const HostVar* w = nullptr;
            if (find_var(ctx, l.name + "/weights", &w) == 0) pack_conv16(l, w->data.data(), h16.data());
        }
        if (!ctx->blob16) CHK(dev_realloc(ctx, &ctx->blob16, ctx->T.blob16_halves));
        HIPCHK(ctx, hipMemcpy(ctx->blob16, h16.data(), sizeof(hp3d_f16) * ctx->T.blob16_halves, hipMemcpyHostToDevice));
    }
    // raw HWIO copies for the debug conv (conv_impl=naive)
    if (ctx->conv_naive)
        for (const ConvL& l : ctx->T.conv) {
            const HostVar* w = nullptr;
            if (find_var(ctx, l.name + "/weights", &w) != 0) continue;
            float* d = nullptr;
            HIPCHK(ctx, hipMalloc((void**)&d, w->data.size() * sizeof(float)));
            HIPCHK(ctx, hipMemcpy(d, w->data.data(), w->data.size() * sizeof(float), hipMemcpyHostToDevice));
            if (ctx->naive_w.count(l.name)) hipFree(ctx->naive_w[l.name]);
            ctx->naive_w[l.name] = d;
        }
    return 0;
}

// blob = [float32 section (all nets) | float16 section (trunk filters, always reserved so every rank agrees on the size)]
int hp3d_weights_blob_bytes(hp3d_ctx* ctx, size_t* bytes) {
    if (!ctx || !bytes) return HP3D_ERR_ARG;
    *bytes = ctx->T.blob_floats * sizeof(float) + ctx->T.blob16_halves * sizeof(hp3d_f16);
    return 0;
}
int hp3d_weights_blob_export(hp3d_ctx* ctx, void* dev_dst) {
    if (!ctx || !dev_dst) return HP3D_ERR_ARG;
    if (!ctx->blob) HP3D_FAIL(ctx, HP3D_ERR_WEIGHTS, "weights not finalized");
    const size_t n32 = ctx->T.blob_floats * sizeof(float), n16 = ctx->T.blob16_halves * sizeof(hp3d_f16);
    HIPCHK(ctx, hipMemcpyAsync(dev_dst, ctx->blob, n32, hipMemcpyDeviceToDevice, ctx->stream));
    if (ctx->blob16)
        HIPCHK(ctx, hipMemcpyAsync((char*)dev_dst + n32, ctx->blob16, n16, hipMemcpyDeviceToDevice, ctx->stream));
    else
        HIPCHK(ctx, hipMemsetAsync((char*)dev_dst + n32, 0, n16, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}
int hp3d_weights_blob_import(hp3d_ctx* ctx, const void* dev_src, int nets_mask) {
    if (ctx) ++ctx->graph_epoch;
    if (!ctx || !dev_src) return HP3D_ERR_ARG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t n32 = ctx->T.blob_floats * sizeof(float), n16 = ctx->T.blob16_halves * sizeof(hp3d_f16);
    if (!ctx->blob) CHK(dev_realloc(ctx, &ctx->blob, ctx->T.blob_floats));
    HIPCHK(ctx, hipMemcpyAsync(ctx->blob, dev_src, n32, hipMemcpyDeviceToDevice, ctx->stream));
    const int f16 = (nets_mask & 32) ? 1 : 0;     // bit 5: the half-precision section is live (dtype 1)
    if (f16) {
        if (!ctx->blob16) CHK(dev_realloc(ctx, &ctx->blob16, ctx->T.blob16_halves));
        HIPCHK(ctx, hipMemcpyAsync(ctx->blob16, (const char*)dev_src + n32, n16, hipMemcpyDeviceToDevice, ctx->stream));
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->nets = nets_mask & 31;
    ctx->prec = f16;
    return 0;
}
int hp3d_nets_mask(hp3d_ctx* ctx) { return ctx ? (ctx->nets | (ctx->prec ? 32 : 0)) : 0; }

int hp3d_infer_full(hp3d_ctx* ctx, int B, int H, int W, const float* image, const float* hand_side,
                    float* hand_scoremap, float* image_crop, float* scale_crop, float* center,
                    float* keypoints_scoremap, float* keypoint_coord3d, float* hand_mask) {
    return infer_full_chunked(ctx, B, H, W, image, hand_side, hand_scoremap, image_crop, scale_crop, center,
                              keypoints_scoremap, keypoint_coord3d, hand_mask, false);
}
int hp3d_infer_full_dev(hp3d_ctx* ctx, int B, int H, int W, const float* image, const float* hand_side,
                        float* hand_scoremap, float* image_crop, float* scale_crop, float* center,
                        float* keypoints_scoremap, float* keypoint_coord3d, float* hand_mask) {
    if (!ctx) return HP3D_ERR_ARG;
    return run_graphed(ctx, graph_key("full", {B, H, W}, {image, hand_side, hand_scoremap, image_crop, scale_crop, center,
                                                        keypoints_scoremap, keypoint_coord3d, hand_mask}), [&]() {
        return infer_full_chunked(ctx, B, H, W, image, hand_side, hand_scoremap, image_crop, scale_crop, center,
                                  keypoints_scoremap, keypoint_coord3d, hand_mask, true);
    });
}

int hp3d_infer_full_kp(hp3d_ctx* ctx, int B, int H, int W, const float* image, const float* hand_side,
                       float* hand_scoremap, float* image_crop, float* scale_crop, float* center,
                       float* keypoints_scoremap, float* keypoint_coord3d, float* hand_mask,
                       int32_t* keypoint_hw_crop, double* keypoint_hw) {
    return infer_full_chunked(ctx, B, H, W, image, hand_side, hand_scoremap, image_crop, scale_crop, center,
                              keypoints_scoremap, keypoint_coord3d, hand_mask, false, nullptr, 0, 0, keypoint_hw_crop, keypoint_hw);
}
int hp3d_infer_full_kp_dev(hp3d_ctx* ctx, int B, int H, int W, const float* image, const float* hand_side,
                           float* hand_scoremap, float* image_crop, float* scale_crop, float* center,
                           float* keypoints_scoremap, float* keypoint_coord3d, float* hand_mask,
                           int32_t* keypoint_hw_crop, double* keypoint_hw) {
    if (!ctx) return HP3D_ERR_ARG;
    return run_graphed(ctx, graph_key("fullkp", {B, H, W}, {image, hand_side, hand_scoremap, image_crop, scale_crop, center,
                                                          keypoints_scoremap, keypoint_coord3d, hand_mask, keypoint_hw_crop, keypoint_hw}), [&]() {
        return infer_full_chunked(ctx, B, H, W, image, hand_side, hand_scoremap, image_crop, scale_crop, center,
                                  keypoints_scoremap, keypoint_coord3d, hand_mask, true, nullptr, 0, 0, keypoint_hw_crop, keypoint_hw);
    });
}
int hp3d_infer_full_kp_u8(hp3d_ctx* ctx, int B, int Hin, int Win, const uint8_t* image_u8, int H, int W,
                          const float* hand_side, float* hand_scoremap, float* image_crop, float* scale_crop,
                          float* center, float* keypoints_scoremap, float* keypoint_coord3d, float* hand_mask,
                          int32_t* keypoint_hw_crop, double* keypoint_hw) {
    return infer_full_chunked(ctx, B, H, W, nullptr, hand_side, hand_scoremap, image_crop, scale_crop, center,
                              keypoints_scoremap, keypoint_coord3d, hand_mask, false, image_u8, Hin, Win, keypoint_hw_crop, keypoint_hw);
}

int hp3d_infer_full_u8(hp3d_ctx* ctx, int B, int Hin, int Win, const uint8_t* image_u8, int H, int W,
                       const float* hand_side, float* hand_scoremap, float* image_crop, float* scale_crop,
                       float* center, float* keypoints_scoremap, float* keypoint_coord3d, float* hand_mask) {
    return infer_full_chunked(ctx, B, H, W, nullptr, hand_side, hand_scoremap, image_crop, scale_crop, center,
                              keypoints_scoremap, keypoint_coord3d, hand_mask, false, image_u8, Hin, Win);
}

// ---- several hands per frame ------------------------------------------------------------------------------
int hp3d_infer_hands(hp3d_ctx* ctx, int B, int H, int W, int K, const float* image, const float* hand_side, float* hand_scoremap,
                     float* image_crop, float* scale_crop, float* center, float* keypoints_scoremap, float* keypoint_coord3d,
                     float* hand_mask, int32_t* keypoint_hw_crop, double* keypoint_hw, int32_t* valid, int32_t* area) {
    if (!ctx) return HP3D_ERR_ARG;
    if (!image) HP3D_FAIL(ctx, HP3D_ERR_ARG, "image / hand_side is NULL");
    return infer_hands_impl(ctx, B, H, W, K, StepIn{image, nullptr, nullptr, hand_side, false}, 0, 0,
                            StepOut{image_crop, scale_crop, center, keypoints_scoremap, keypoint_coord3d, keypoint_hw_crop, keypoint_hw,
                                    nullptr, nullptr, nullptr, valid, area}, hand_scoremap, hand_mask);
}
int hp3d_infer_hands_dev(hp3d_ctx* ctx, int B, int H, int W, int K, const float* image, const float* hand_side, float* hand_scoremap,
                         float* image_crop, float* scale_crop, float* center, float* keypoints_scoremap, float* keypoint_coord3d,
                         float* hand_mask, int32_t* keypoint_hw_crop, double* keypoint_hw, int32_t* valid, int32_t* area) {
    if (!ctx) return HP3D_ERR_ARG;
    if (!image) HP3D_FAIL(ctx, HP3D_ERR_ARG, "image / hand_side is NULL");
    return infer_hands_impl(ctx, B, H, W, K, StepIn{image, nullptr, nullptr, hand_side, true}, 0, 0,
                            StepOut{image_crop, scale_crop, center, keypoints_scoremap, keypoint_coord3d, keypoint_hw_crop, keypoint_hw,
                                    nullptr, nullptr, nullptr, valid, area}, hand_scoremap, hand_mask);
}
int hp3d_infer_hands_u8(hp3d_ctx* ctx, int B, int Hin, int Win, const uint8_t* image_u8, int H, int W, int K, const float* hand_side,
                        float* hand_scoremap, float* image_crop, float* scale_crop, float* center, float* keypoints_scoremap,
                        float* keypoint_coord3d, float* hand_mask, int32_t* keypoint_hw_crop, double* keypoint_hw, int32_t* valid,
                        int32_t* area) {
    if (!ctx) return HP3D_ERR_ARG;
    if (!image_u8) HP3D_FAIL(ctx, HP3D_ERR_ARG, "image / hand_side is NULL");
    return infer_hands_impl(ctx, B, H, W, K, StepIn{nullptr, image_u8, nullptr, hand_side, false}, Hin, Win,
                            StepOut{image_crop, scale_crop, center, keypoints_scoremap, keypoint_coord3d, keypoint_hw_crop, keypoint_hw,
                                    nullptr, nullptr, nullptr, valid, area}, hand_scoremap, hand_mask);
}

static int masks_from_scoremap_impl(hp3d_ctx* ctx, const float* scoremap, int B, int H, int W, int K, const int32_t* keep,
                                    const float* keep_center, const float* keep_scale, float* mask, float* center, float* crop_size,
                                    float* scale, int32_t* seed, int32_t* valid, int32_t* area, int32_t* claimed) {
    if (!ctx) return HP3D_ERR_ARG;
    if (!scoremap || B < 1 || H < 1 || W < 1) HP3D_FAIL(ctx, HP3D_ERR_ARG, "bad arguments");
    if (K < 1 || K > HP3D_MAX_HANDS) HP3D_FAIL(ctx, HP3D_ERR_ARG, "max hands K=%d must be in 1 ... %d", K, HP3D_MAX_HANDS);
    if (!(B < H && B < W)) HP3D_FAIL(ctx, HP3D_ERR_ARG, "Scoremap must be [Batch, Width, Height]");  // general.py:210
    if ((long)H * W > (1L << 30)) HP3D_FAIL(ctx, HP3D_ERR_ARG, "map too large (more than 2^30 pixels)");
    const bool global = mask_grow_global(ctx, H, W);
    if (!global && !mask_grow_lds_fits(H, W)) HP3D_FAIL(ctx, HP3D_ERR_ARG, "map too large for the in-LDS mask growth");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Scratch S(ctx);
    const size_t npx = (size_t)B * H * W, ns = (size_t)B * K;
    float* d_sm = S.upload(scoremap, npx * 2); NN(ctx, d_sm);
    MaskBuffers mb;
    mb.argmax_key = S.alloc<unsigned long long>(B); NN(ctx, mb.argmax_key);
    mb.det = S.alloc<unsigned char>(npx); NN(ctx, mb.det);
    mb.fg = S.alloc<float>(npx); NN(ctx, mb.fg);
    float* d_mask = nullptr;
    if (mask) { d_mask = S.alloc<float>(ns * H * W); NN(ctx, d_mask); }
    float* d_c = S.alloc<float>(ns * 2); NN(ctx, d_c);
    float* d_cs = S.alloc<float>(ns); NN(ctx, d_cs);
    float* d_sc = S.alloc<float>(ns); NN(ctx, d_sc);
    int* d_seed = S.alloc<int>(ns * 2); NN(ctx, d_seed);
    int* d_valid = S.alloc<int>(ns); NN(ctx, d_valid);
    int* d_area = S.alloc<int>(ns); NN(ctx, d_area);
    unsigned* d_scr = nullptr;
    if (global) { d_scr = S.alloc<unsigned>((size_t)B * mask_grow_global_words(H, W)); NN(ctx, d_scr); }
    MaskKeep mk;
    int* d_claimed = nullptr;
    if (keep) {
        mk.keep = S.upload((const int*)keep, ns); NN(ctx, mk.keep);
        mk.center = S.upload(keep_center, ns * 2); NN(ctx, mk.center);
        mk.scale = S.upload(keep_scale, ns); NN(ctx, mk.scale);
        d_claimed = S.alloc<int>(ns); NN(ctx, d_claimed);
        mk.claimed = d_claimed;
    }
    seg_softmax_launch(d_sm, B, H, W, mb, ctx->stream);
    mask_grow_multi_launch(mb, B, H, W, K, ctx->hands_min_area, ctx->empty_fltmax, d_scr, d_mask, d_c, d_cs, d_sc, d_seed, d_valid, d_area,
                           ctx->stream, mk);
    ++ctx->mask_grow_multi_launches;
    if (global) ++ctx->mask_grow_global_launches;
    if (mask) HIPCHK(ctx, hipMemcpyAsync(mask, d_mask, ns * H * W * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    if (center) HIPCHK(ctx, hipMemcpyAsync(center, d_c, sizeof(float) * ns * 2, hipMemcpyDeviceToHost, ctx->stream));
    if (crop_size) HIPCHK(ctx, hipMemcpyAsync(crop_size, d_cs, sizeof(float) * ns, hipMemcpyDeviceToHost, ctx->stream));
    if (scale) HIPCHK(ctx, hipMemcpyAsync(scale, d_sc, sizeof(float) * ns, hipMemcpyDeviceToHost, ctx->stream));
    if (seed) HIPCHK(ctx, hipMemcpyAsync(seed, d_seed, sizeof(int) * ns * 2, hipMemcpyDeviceToHost, ctx->stream));
    if (valid) HIPCHK(ctx, hipMemcpyAsync(valid, d_valid, sizeof(int) * ns, hipMemcpyDeviceToHost, ctx->stream));
    if (area) HIPCHK(ctx, hipMemcpyAsync(area, d_area, sizeof(int) * ns, hipMemcpyDeviceToHost, ctx->stream));
    if (claimed && d_claimed) HIPCHK(ctx, hipMemcpyAsync(claimed, d_claimed, sizeof(int) * ns, hipMemcpyDeviceToHost, ctx->stream));
    return finish_op(ctx);
}

int hp3d_masks_from_scoremap(hp3d_ctx* ctx, const float* scoremap, int B, int H, int W, int K, float* mask, float* center,
                             float* crop_size, float* scale, int32_t* seed, int32_t* valid, int32_t* area) {
    return masks_from_scoremap_impl(ctx, scoremap, B, H, W, K, nullptr, nullptr, nullptr, mask, center, crop_size, scale, seed, valid, area,
                                    nullptr);
}

int hp3d_masks_from_scoremap_keep(hp3d_ctx* ctx, const float* scoremap, int B, int H, int W, int K, const int32_t* keep,
                                  const float* keep_center, const float* keep_scale, float* mask, float* center, float* crop_size,
                                  float* scale, int32_t* seed, int32_t* valid, int32_t* area, int32_t* claimed) {
    if (!ctx) return HP3D_ERR_ARG;
    if (!keep || !keep_center || !keep_scale) HP3D_FAIL(ctx, HP3D_ERR_ARG, "keep / keep_center / keep_scale is NULL");
    return masks_from_scoremap_impl(ctx, scoremap, B, H, W, K, keep, keep_center, keep_scale, mask, center, crop_size, scale, seed, valid,
                                    area, claimed);
}

// ---- tracking several hands per frame --------------------------------------------------------------------
int hp3d_track_hands_reset(hp3d_ctx* ctx) {
    if (!ctx) return HP3D_ERR_ARG;
    ctx->track_hands.ok = false;
    ctx->track_hands.since = 0;
    return 0;
}

int hp3d_track_hands_seed(hp3d_ctx* ctx, int B, int H, int W, int K, const float* center, const float* scale, const int32_t* valid) {
    if (!ctx) return HP3D_ERR_ARG;
    if (!center || !scale || !valid) HP3D_FAIL(ctx, HP3D_ERR_ARG, "center / scale / valid is NULL");
    if (K < 1 || K > HP3D_MAX_HANDS) HP3D_FAIL(ctx, HP3D_ERR_ARG, "max hands K=%d must be in 1 ... %d", K, HP3D_MAX_HANDS);
    CHK(check_img(ctx, B, H, W));
    const int n = B * K;
    // an absent slot crops with the fall-back box an empty mask gives (mask_grow_epilogue, option "empty_reduce")
    const float fb_c = ctx->empty_fltmax ? 0.f : 160.f, fb_s = fminf(fmaxf(256.0f / (100.f * 1.25f), 0.25f), 5.0f);
    std::vector<float> c(center, center + (size_t)n * 2), s(scale, scale + n);
    std::vector<int> v(n);
    for (int b = 0; b < B; ++b) {
        bool any = false;
        for (int j = 0; j < K; ++j) {
            const int i = b * K + j;
            v[i] = valid[i] != 0 ? 1 : 0;
            if (!v[i]) { c[i * 2] = c[i * 2 + 1] = fb_c; s[i] = fb_s; continue; }
            any = true;
            if (!(scale[i] > 0.f) || !std::isfinite(scale[i])) HP3D_FAIL(ctx, HP3D_ERR_ARG, "track_hands_seed: scale[%d,%d] = %g must be positive and finite", b, j, (double)scale[i]);
            if (!std::isfinite(center[i * 2]) || !std::isfinite(center[i * 2 + 1])) HP3D_FAIL(ctx, HP3D_ERR_ARG, "track_hands_seed: center[%d,%d] is not finite", b, j);
        }
        if (!any) HP3D_FAIL(ctx, HP3D_ERR_ARG, "track_hands_seed: image %d has no valid slot", b);
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    CHK(ensure_track_hands(ctx, n));
    TrackHandsState& T = ctx->track_hands;
    CHK(T.h_flags.wait(ctx));
    T.ok = false;
    T.B = B; T.K = K; T.H = H; T.W = W; T.f = ctx->detect_scale;
    HIPCHK(ctx, hipMemcpyAsync(T.center[T.cur], c.data(), sizeof(float) * (size_t)n * 2, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(T.scale[T.cur], s.data(), sizeof(float) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(T.valid(), v.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(T.keep, v.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(T.lost(), 0, sizeof(int) * (size_t)n, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < n; ++i) { T.h_flags.h[i] = v[i]; T.h_flags.h[n + i] = 0; }
    T.ok = true; T.since = 0;
    return 0;
}

int hp3d_track_hands_step(hp3d_ctx* ctx, int B, int H, int W, int K, const float* image, const float* hand_side, float* image_crop,
                          float* scale_crop, float* center, float* keypoints_scoremap, float* keypoint_coord3d, int32_t* keypoint_hw_crop,
                          double* keypoint_hw, float* confidence, int32_t* lost, int32_t* detected, int32_t* valid, int32_t* area,
                          int32_t* claimed) {
    if (!ctx) return HP3D_ERR_ARG;
    if (!image) HP3D_FAIL(ctx, HP3D_ERR_ARG, "image / hand_side is NULL");
    return track_hands_step_impl(ctx, B, H, W, K, StepIn{image, nullptr, nullptr, hand_side, false},
                                 StepOut{image_crop, scale_crop, center, keypoints_scoremap, keypoint_coord3d, keypoint_hw_crop,
                                         keypoint_hw, confidence, lost, detected, valid, area, claimed});
}
int hp3d_track_hands_step_dev(hp3d_ctx* ctx, int B, int H, int W, int K, const float* image, const float* hand_side, float* image_crop,
                              float* scale_crop, float* center, float* keypoints_scoremap, float* keypoint_coord3d,
                              int32_t* keypoint_hw_crop, double* keypoint_hw, float* confidence, int32_t* lost, int32_t* detected,
                              int32_t* valid, int32_t* area, int32_t* claimed) {
    if (!ctx) return HP3D_ERR_ARG;
    if (!image) HP3D_FAIL(ctx, HP3D_ERR_ARG, "image / hand_side is NULL");
    return track_hands_step_impl(ctx, B, H, W, K, StepIn{image, nullptr, nullptr, hand_side, true},
                                 StepOut{image_crop, scale_crop, center, keypoints_scoremap, keypoint_coord3d, keypoint_hw_crop,
                                         keypoint_hw, confidence, lost, detected, valid, area, claimed});
}
int hp3d_track_hands_step_u8(hp3d_ctx* ctx, int B, int Hin, int Win, const uint8_t* image_u8, int H, int W, int K, const float* hand_side,
                             float* image_crop, float* scale_crop, float* center, float* keypoints_scoremap, float* keypoint_coord3d,
                             int32_t* keypoint_hw_crop, double* keypoint_hw, float* confidence, int32_t* lost, int32_t* detected,
                             int32_t* valid, int32_t* area, int32_t* claimed) {
    if (!ctx) return HP3D_ERR_ARG;
    if (!image_u8) HP3D_FAIL(ctx, HP3D_ERR_ARG, "image / hand_side is NULL");
    if (Hin != H || Win != W)
        HP3D_FAIL(ctx, HP3D_ERR_UNSUPPORTED, "tracking crops straight from the uint8 frame: the frame (%dx%d) must have the network size (%dx%d)", Hin, Win, H, W);
    return track_hands_step_impl(ctx, B, H, W, K, StepIn{nullptr, image_u8, nullptr, hand_side, false},
                                 StepOut{image_crop, scale_crop, center, keypoints_scoremap, keypoint_coord3d, keypoint_hw_crop,
                                         keypoint_hw, confidence, lost, detected, valid, area, claimed});
}

int hp3d_track_hands_step_nv12(hp3d_ctx* ctx, int B, int H, int W, const uint8_t* y, const uint8_t* uv, int pitch, int64_t frame_stride, int K,
                               const float* hand_side, float* image_crop, float* scale_crop, float* center, float* keypoints_scoremap,
                               float* keypoint_coord3d, int32_t* keypoint_hw_crop, double* keypoint_hw, float* confidence, int32_t* lost,
                               int32_t* detected, int32_t* valid, int32_t* area, int32_t* claimed) {
    if (!ctx) return HP3D_ERR_ARG;
    const Nv12Arg nv{y, uv, pitch, (long long)frame_stride};
    return track_hands_step_impl(ctx, B, H, W, K, StepIn{nullptr, nullptr, &nv, hand_side, false},
                                 StepOut{image_crop, scale_crop, center, keypoints_scoremap, keypoint_coord3d, keypoint_hw_crop,
                                         keypoint_hw, confidence, lost, detected, valid, area, claimed});
}
int hp3d_track_hands_step_nv12_dev(hp3d_ctx* ctx, int B, int H, int W, const uint8_t* y, const uint8_t* uv, int pitch, int64_t frame_stride,
                                   int K, const float* hand_side, float* image_crop, float* scale_crop, float* center,
                                   float* keypoints_scoremap, float* keypoint_coord3d, int32_t* keypoint_hw_crop, double* keypoint_hw,
                                   float* confidence, int32_t* lost, int32_t* detected, int32_t* valid, int32_t* area, int32_t* claimed) {
    if (!ctx) return HP3D_ERR_ARG;
    const Nv12Arg nv{y, uv, pitch, (long long)frame_stride};
    return track_hands_step_impl(ctx, B, H, W, K, StepIn{nullptr, nullptr, &nv, hand_side, true},
                                 StepOut{image_crop, scale_crop, center, keypoints_scoremap, keypoint_coord3d, keypoint_hw_crop,
                                         keypoint_hw, confidence, lost, detected, valid, area, claimed});
}

int hp3d_track_hands_step_px(hp3d_ctx* ctx, int B, int H, int W, const uint8_t* px, int pitch, int64_t frame_stride, int format, int K,
                             const float* hand_side, float* image_crop, float* scale_crop, float* center, float* keypoints_scoremap,
                             float* keypoint_coord3d, int32_t* keypoint_hw_crop, double* keypoint_hw, float* confidence, int32_t* lost,
                             int32_t* detected, int32_t* valid, int32_t* area, int32_t* claimed) {
    if (!ctx) return HP3D_ERR_ARG;
    const PxArg pa{px, pitch, (long long)frame_stride, format};
    return track_hands_step_impl(ctx, B, H, W, K, StepIn{nullptr, nullptr, nullptr, hand_side, false, &pa},
                                 StepOut{image_crop, scale_crop, center, keypoints_scoremap, keypoint_coord3d, keypoint_hw_crop,
                                         keypoint_hw, confidence, lost, detected, valid, area, claimed});
}
int hp3d_track_hands_step_px_dev(hp3d_ctx* ctx, int B, int H, int W, const uint8_t* px, int pitch, int64_t frame_stride, int format, int K,
                                 const float* hand_side, float* image_crop, float* scale_crop, float* center, float* keypoints_scoremap,
                                 float* keypoint_coord3d, int32_t* keypoint_hw_crop, double* keypoint_hw, float* confidence, int32_t* lost,
                                 int32_t* detected, int32_t* valid, int32_t* area, int32_t* claimed) {
    if (!ctx) return HP3D_ERR_ARG;
    const PxArg pa{px, pitch, (long long)frame_stride, format};
    return track_hands_step_impl(ctx, B, H, W, K, StepIn{nullptr, nullptr, nullptr, hand_side, true, &pa},
                                 StepOut{image_crop, scale_crop, center, keypoints_scoremap, keypoint_coord3d, keypoint_hw_crop,
                                         keypoint_hw, confidence, lost, detected, valid, area, claimed});
}

int hp3d_track_hands_step_surf(hp3d_ctx* ctx, int B, int H, int W, const hp3d_surface* surfaces, int K, const float* hand_side,
                               float* image_crop, float* scale_crop, float* center, float* keypoints_scoremap, float* keypoint_coord3d,
                               int32_t* keypoint_hw_crop, double* keypoint_hw, float* confidence, int32_t* lost, int32_t* detected,
                               int32_t* valid, int32_t* area, int32_t* claimed) {
    if (!ctx) return HP3D_ERR_ARG;
    if (!surfaces) HP3D_FAIL(ctx, HP3D_ERR_ARG, "surf: surfaces is NULL");
    return track_hands_step_impl(ctx, B, H, W, K, StepIn{nullptr, nullptr, nullptr, hand_side, false, nullptr, surfaces},
                                 StepOut{image_crop, scale_crop, center, keypoints_scoremap, keypoint_coord3d, keypoint_hw_crop,
                                         keypoint_hw, confidence, lost, detected, valid, area, claimed});
}
int hp3d_track_hands_step_surf_dev(hp3d_ctx* ctx, int B, int H, int W, const hp3d_surface* surfaces, int K, const float* hand_side,
                                   float* image_crop, float* scale_crop, float* center, float* keypoints_scoremap, float* keypoint_coord3d,
                                   int32_t* keypoint_hw_crop, double* keypoint_hw, float* confidence, int32_t* lost, int32_t* detected,
                                   int32_t* valid, int32_t* area, int32_t* claimed) {
    if (!ctx) return HP3D_ERR_ARG;
    if (!surfaces) HP3D_FAIL(ctx, HP3D_ERR_ARG, "surf: surfaces is NULL");
    return track_hands_step_impl(ctx, B, H, W, K, StepIn{nullptr, nullptr, nullptr, hand_side, true, nullptr, surfaces},
                                 StepOut{image_crop, scale_crop, center, keypoints_scoremap, keypoint_coord3d, keypoint_hw_crop,
                                         keypoint_hw, confidence, lost, detected, valid, area, claimed});
}

int hp3d_track_hands_box(hp3d_ctx* ctx, int B, int K, int H, int W, const double* keypoint_hw, const float* score32, float margin,
                         const int32_t* valid, const float* box_center, const float* box_scale, float* center, float* scale,
                         float* confidence, int32_t* lost) {
    if (!ctx) return HP3D_ERR_ARG;
    if (!keypoint_hw || !valid || !box_center || !box_scale || !center || !scale || !confidence || !lost || B < 1 || H < 1 || W < 1)
        HP3D_FAIL(ctx, HP3D_ERR_ARG, "bad arguments");
    if (K < 1 || K > HP3D_MAX_HANDS) HP3D_FAIL(ctx, HP3D_ERR_ARG, "max hands K=%d must be in 1 ... %d", K, HP3D_MAX_HANDS);
    if (!(margin >= 0.f && margin <= 16.f)) HP3D_FAIL(ctx, HP3D_ERR_ARG, "track_hands_box: margin %g must be 0 (= option track_margin) or in (0, 16]", (double)margin);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Scratch S(ctx);
    const size_t n = (size_t)B * K;
    double* d_kp = S.upload(keypoint_hw, n * 42); NN(ctx, d_kp);
    float* d_sm = nullptr;
    if (score32) { d_sm = S.upload(score32, n * 32 * 32 * 21); NN(ctx, d_sm); }
    int* d_v = S.upload((const int*)valid, n); NN(ctx, d_v);
    float* d_bc = S.upload(box_center, n * 2); NN(ctx, d_bc);
    float* d_bs = S.upload(box_scale, n); NN(ctx, d_bs);
    float* d_c = S.alloc<float>(n * 2); NN(ctx, d_c);
    float* d_s = S.alloc<float>(n); NN(ctx, d_s);
    float* d_q = S.alloc<float>(n); NN(ctx, d_q);
    int* d_l = S.alloc<int>(n); NN(ctx, d_l);
    track_hands_box_launch(d_kp, d_sm, 21, (int)n, H, W, 256, margin > 0.f ? margin : ctx->track_margin, ctx->track_min_score,
                           ctx->track_use_min_score, d_v, d_bc, d_bs, d_c, d_s, d_q, d_l, nullptr, nullptr, nullptr, nullptr, ctx->stream);
    HIPCHK(ctx, hipMemcpyAsync(center, d_c, sizeof(float) * n * 2, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(scale, d_s, sizeof(float) * n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(confidence, d_q, sizeof(float) * n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(lost, d_l, sizeof(int) * n, hipMemcpyDeviceToHost, ctx->stream));
    return finish_op(ctx);
}

// ---- tracking: hands across video frames ----------------------------------------------------------------
int hp3d_track_reset(hp3d_ctx* ctx) {
    if (!ctx) return HP3D_ERR_ARG;
    ctx->track.valid = false;
    ctx->track.since = 0;
    return 0;
}

int hp3d_track_seed(hp3d_ctx* ctx, int B, int H, int W, const float* center, const float* scale) {
    if (!ctx) return HP3D_ERR_ARG;
    if (!center || !scale) HP3D_FAIL(ctx, HP3D_ERR_ARG, "center / scale is NULL");
    CHK(check_img(ctx, B, H, W));
    for (int b = 0; b < B; ++b) {
        if (!(scale[b] > 0.f) || !std::isfinite(scale[b])) HP3D_FAIL(ctx, HP3D_ERR_ARG, "track_seed: scale[%d] = %g must be positive and finite", b, (double)scale[b]);
        if (!std::isfinite(center[b * 2]) || !std::isfinite(center[b * 2 + 1])) HP3D_FAIL(ctx, HP3D_ERR_ARG, "track_seed: center[%d] is not finite", b);
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    CHK(ensure_track(ctx, B));
    TrackState& T = ctx->track;
    CHK(T.h_lost.wait(ctx));
    HIPCHK(ctx, hipMemcpyAsync(T.center[T.cur], center, sizeof(float) * (size_t)B * 2, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(T.scale[T.cur], scale, sizeof(float) * (size_t)B, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(T.lost, 0, sizeof(int) * (size_t)B, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    for (int b = 0; b < B; ++b) T.h_lost.h[b] = 0;
    T.valid = true; T.B = B; T.H = H; T.W = W; T.f = ctx->detect_scale; T.since = 0;
    return 0;
}

int hp3d_track_step(hp3d_ctx* ctx, int B, int H, int W, const float* image, const float* hand_side, float* image_crop,
                    float* scale_crop, float* center, float* keypoints_scoremap, float* keypoint_coord3d,
                    int32_t* keypoint_hw_crop, double* keypoint_hw, float* confidence, int32_t* lost, int32_t* detected) {
    if (!ctx) return HP3D_ERR_ARG;
    if (!image) HP3D_FAIL(ctx, HP3D_ERR_ARG, "image / hand_side is NULL");
    return track_step_impl(ctx, B, H, W, StepIn{image, nullptr, nullptr, hand_side, false},
                           StepOut{image_crop, scale_crop, center, keypoints_scoremap, keypoint_coord3d, keypoint_hw_crop, keypoint_hw,
                                   confidence, lost, detected});
}
int hp3d_track_step_dev(hp3d_ctx* ctx, int B, int H, int W, const float* image, const float* hand_side, float* image_crop,
                        float* scale_crop, float* center, float* keypoints_scoremap, float* keypoint_coord3d,
                        int32_t* keypoint_hw_crop, double* keypoint_hw, float* confidence, int32_t* lost, int32_t* detected) {
    if (!ctx) return HP3D_ERR_ARG;
    if (!image) HP3D_FAIL(ctx, HP3D_ERR_ARG, "image / hand_side is NULL");
    return track_step_impl(ctx, B, H, W, StepIn{image, nullptr, nullptr, hand_side, true},
                           StepOut{image_crop, scale_crop, center, keypoints_scoremap, keypoint_coord3d, keypoint_hw_crop, keypoint_hw,
                                   confidence, lost, detected});
}
int hp3d_track_step_u8(hp3d_ctx* ctx, int B, int Hin, int Win, const uint8_t* image_u8, int H, int W, const float* hand_side,
                       float* image_crop, float* scale_crop, float* center, float* keypoints_scoremap, float* keypoint_coord3d,
                       int32_t* keypoint_hw_crop, double* keypoint_hw, float* confidence, int32_t* lost, int32_t* detected) {
    if (!ctx) return HP3D_ERR_ARG;
    if (!image_u8) HP3D_FAIL(ctx, HP3D_ERR_ARG, "image / hand_side is NULL");
    if (Hin != H || Win != W)
        HP3D_FAIL(ctx, HP3D_ERR_UNSUPPORTED, "tracking crops straight from the uint8 frame: the frame (%dx%d) must have the network size (%dx%d)", Hin, Win, H, W);
    return track_step_impl(ctx, B, H, W, StepIn{nullptr, image_u8, nullptr, hand_side, false},
                           StepOut{image_crop, scale_crop, center, keypoints_scoremap, keypoint_coord3d, keypoint_hw_crop, keypoint_hw,
                                   confidence, lost, detected});
}

int hp3d_track_step_nv12(hp3d_ctx* ctx, int B, int H, int W, const uint8_t* y, const uint8_t* uv, int pitch, int64_t frame_stride,
                         const float* hand_side, float* image_crop, float* scale_crop, float* center, float* keypoints_scoremap,
                         float* keypoint_coord3d, int32_t* keypoint_hw_crop, double* keypoint_hw, float* confidence, int32_t* lost,
                         int32_t* detected) {
    if (!ctx) return HP3D_ERR_ARG;
    const Nv12Arg nv{y, uv, pitch, (long long)frame_stride};
    return track_step_impl(ctx, B, H, W, StepIn{nullptr, nullptr, &nv, hand_side, false},
                           StepOut{image_crop, scale_crop, center, keypoints_scoremap, keypoint_coord3d, keypoint_hw_crop, keypoint_hw,
                                   confidence, lost, detected});
}
int hp3d_track_step_nv12_dev(hp3d_ctx* ctx, int B, int H, int W, const uint8_t* y, const uint8_t* uv, int pitch, int64_t frame_stride,
                             const float* hand_side, float* image_crop, float* scale_crop, float* center, float* keypoints_scoremap,
                             float* keypoint_coord3d, int32_t* keypoint_hw_crop, double* keypoint_hw, float* confidence, int32_t* lost,
                             int32_t* detected) {
    if (!ctx) return HP3D_ERR_ARG;
    const Nv12Arg nv{y, uv, pitch, (long long)frame_stride};
    return track_step_impl(ctx, B, H, W, StepIn{nullptr, nullptr, &nv, hand_side, true},
                           StepOut{image_crop, scale_crop, center, keypoints_scoremap, keypoint_coord3d, keypoint_hw_crop, keypoint_hw,
                                   confidence, lost, detected});
}

int hp3d_track_step_px(hp3d_ctx* ctx, int B, int H, int W, const uint8_t* px, int pitch, int64_t frame_stride, int format,
                       const float* hand_side, float* image_crop, float* scale_crop, float* center, float* keypoints_scoremap,
                       float* keypoint_coord3d, int32_t* keypoint_hw_crop, double* keypoint_hw, float* confidence, int32_t* lost,
                       int32_t* detected) {
    if (!ctx) return HP3D_ERR_ARG;
    const PxArg pa{px, pitch, (long long)frame_stride, format};
    return track_step_impl(ctx, B, H, W, StepIn{nullptr, nullptr, nullptr, hand_side, false, &pa},
                           StepOut{image_crop, scale_crop, center, keypoints_scoremap, keypoint_coord3d, keypoint_hw_crop, keypoint_hw,
                                   confidence, lost, detected});
}
int hp3d_track_step_px_dev(hp3d_ctx* ctx, int B, int H, int W, const uint8_t* px, int pitch, int64_t frame_stride, int format,
                           const float* hand_side, float* image_crop, float* scale_crop, float* center, float* keypoints_scoremap,
                           float* keypoint_coord3d, int32_t* keypoint_hw_crop, double* keypoint_hw, float* confidence, int32_t* lost,
                           int32_t* detected) {
    if (!ctx) return HP3D_ERR_ARG;
    const PxArg pa{px, pitch, (long long)frame_stride, format};
    return track_step_impl(ctx, B, H, W, StepIn{nullptr, nullptr, nullptr, hand_side, true, &pa},
                           StepOut{image_crop, scale_crop, center, keypoints_scoremap, keypoint_coord3d, keypoint_hw_crop, keypoint_hw,
                                   confidence, lost, detected});
}

int hp3d_track_step_surf(hp3d_ctx* ctx, int B, int H, int W, const hp3d_surface* surfaces, const float* hand_side, float* image_crop,
                         float* scale_crop, float* center, float* keypoints_scoremap, float* keypoint_coord3d, int32_t* keypoint_hw_crop,
                         double* keypoint_hw, float* confidence, int32_t* lost, int32_t* detected) {
    if (!ctx) return HP3D_ERR_ARG;
    if (!surfaces) HP3D_FAIL(ctx, HP3D_ERR_ARG, "surf: surfaces is NULL");
    return track_step_impl(ctx, B, H, W, StepIn{nullptr, nullptr, nullptr, hand_side, false, nullptr, surfaces},
                           StepOut{image_crop, scale_crop, center, keypoints_scoremap, keypoint_coord3d, keypoint_hw_crop, keypoint_hw,
                                   confidence, lost, detected});
}
int hp3d_track_step_surf_dev(hp3d_ctx* ctx, int B, int H, int W, const hp3d_surface* surfaces, const float* hand_side, float* image_crop,
                             float* scale_crop, float* center, float* keypoints_scoremap, float* keypoint_coord3d,
                             int32_t* keypoint_hw_crop, double* keypoint_hw, float* confidence, int32_t* lost, int32_t* detected) {
    if (!ctx) return HP3D_ERR_ARG;
    if (!surfaces) HP3D_FAIL(ctx, HP3D_ERR_ARG, "surf: surfaces is NULL");
    return track_step_impl(ctx, B, H, W, StepIn{nullptr, nullptr, nullptr, hand_side, true, nullptr, surfaces},
                           StepOut{image_crop, scale_crop, center, keypoints_scoremap, keypoint_coord3d, keypoint_hw_crop, keypoint_hw,
                                   confidence, lost, detected});
}

int hp3d_track_box(hp3d_ctx* ctx, int B, int H, int W, const double* keypoint_hw, const float* score32, float margin, float* center,
                   float* scale, float* confidence, int32_t* lost) {
    if (!ctx) return HP3D_ERR_ARG;
    if (!keypoint_hw || !center || !scale || !confidence || !lost || B < 1 || H < 1 || W < 1) HP3D_FAIL(ctx, HP3D_ERR_ARG, "bad arguments");
    if (!(margin >= 0.f && margin <= 16.f)) HP3D_FAIL(ctx, HP3D_ERR_ARG, "track_box: margin %g must be 0 (= option track_margin) or in (0, 16]", (double)margin);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Scratch S(ctx);
    double* d_kp = S.upload(keypoint_hw, (size_t)B * 42); NN(ctx, d_kp);
    float* d_sm = nullptr;
    if (score32) { d_sm = S.upload(score32, (size_t)B * 32 * 32 * 21); NN(ctx, d_sm); }
    float* d_c = S.alloc<float>((size_t)B * 2); NN(ctx, d_c);
    float* d_s = S.alloc<float>(B); NN(ctx, d_s);
    float* d_q = S.alloc<float>(B); NN(ctx, d_q);
    int* d_l = S.alloc<int>(B); NN(ctx, d_l);
    track_box_launch(d_kp, d_sm, 21, B, H, W, 256, margin > 0.f ? margin : ctx->track_margin, ctx->track_min_score, ctx->track_use_min_score, d_c, d_s, d_q, d_l,
                     nullptr, ctx->stream);
    HIPCHK(ctx, hipMemcpyAsync(center, d_c, sizeof(float) * (size_t)B * 2, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(scale, d_s, sizeof(float) * (size_t)B, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(confidence, d_q, sizeof(float) * (size_t)B, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(lost, d_l, sizeof(int) * (size_t)B, hipMemcpyDeviceToHost, ctx->stream));
    return finish_op(ctx);
}

int hp3d_crop_and_resize_u8(hp3d_ctx* ctx, const uint8_t* image_u8, int B, int H, int W, const float* center,
                            const float* scale, int crop_size, float* out) {
    if (!ctx) return HP3D_ERR_ARG;
    if (!image_u8 || !center || !scale || !out || B < 1 || H < 2 || W < 2 || crop_size < 1) HP3D_FAIL(ctx, HP3D_ERR_ARG, "bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Scratch S(ctx);
    const size_t no = (size_t)B * crop_size * crop_size * 3;
    unsigned char* d_x = S.upload(image_u8, (size_t)B * H * W * 3); NN(ctx, d_x);
    float* d_c = S.upload(center, (size_t)B * 2); NN(ctx, d_c);
    float* d_s = S.upload(scale, (size_t)B); NN(ctx, d_s);
    float* d_o = S.alloc<float>(no); NN(ctx, d_o);
    crop_and_resize_u8_launch(d_x, B, H, W, d_c, d_s, crop_size, d_o, ctx->stream);
    ++ctx->crop_u8_launches;
    HIPCHK(ctx, hipMemcpyAsync(out, d_o, no * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    return finish_op(ctx);
}

// ---- compaction of absent hand slots: the per-op forms -----------------------------------------------------
int hp3d_crop_and_resize_idx(hp3d_ctx* ctx, const float* image, const uint8_t* image_u8, int B, int H, int W, int K, const float* center,
                             const float* scale, const int32_t* idx, int m, int crop_size, float* out) {
    if (!ctx) return HP3D_ERR_ARG;
    if ((!image) == (!image_u8) || !center || !scale || !idx || !out || B < 1 || H < 2 || W < 2 || K < 1 || K > HP3D_MAX_HANDS || m < 0 ||
        m > B * K || crop_size < 1)
        HP3D_FAIL(ctx, HP3D_ERR_ARG, "bad arguments");
    for (int i = 0; i < m; ++i)
        if (idx[i] < 0 || idx[i] >= B * K) HP3D_FAIL(ctx, HP3D_ERR_ARG, "idx[%d] = %d is no slot of %d", i, (int)idx[i], B * K);
    if (m == 0) return 0;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Scratch S(ctx);
    const size_t no = (size_t)m * crop_size * crop_size * 3;
    float* d_c = S.upload(center, (size_t)B * K * 2); NN(ctx, d_c);
    float* d_s = S.upload(scale, (size_t)B * K); NN(ctx, d_s);
    int32_t* d_i = S.upload(idx, (size_t)m); NN(ctx, d_i);
    float* d_o = S.alloc<float>(no); NN(ctx, d_o);
    if (image_u8) {
        unsigned char* d_x = S.upload(image_u8, (size_t)B * H * W * 3); NN(ctx, d_x);
        crop_and_resize_idx_u8_launch(d_x, m, H, W, d_c, d_s, d_i, K, crop_size, d_o, ctx->stream);
        ++ctx->crop_u8_launches;
    } else {
        float* d_x = S.upload(image, (size_t)B * H * W * 3); NN(ctx, d_x);
        crop_and_resize_idx_launch(d_x, m, H, W, 3, d_c, d_s, d_i, K, crop_size, d_o, ctx->stream);
    }
    HIPCHK(ctx, hipMemcpyAsync(out, d_o, no * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    return finish_op(ctx);
}

int hp3d_slot_scatter(hp3d_ctx* ctx, const float* dense, const int32_t* pos, int ns, int m, int words, int skew_words, float* out) {
    if (!ctx) return HP3D_ERR_ARG;
    if (!pos || !out || ns < 1 || m < 0 || m > ns || (m > 0 && !dense) || words < 1 || skew_words < 0 || skew_words > 3)
        HP3D_FAIL(ctx, HP3D_ERR_ARG, "bad arguments");
    for (int s = 0; s < ns; ++s)
        if (pos[s] < -1 || pos[s] >= m) HP3D_FAIL(ctx, HP3D_ERR_ARG, "pos[%d] = %d is no dense index of %d", s, (int)pos[s], m);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Scratch S(ctx);
    const size_t no = (size_t)ns * words + 4;
    float* d_x = S.alloc<float>((size_t)std::max(m, 1) * words); NN(ctx, d_x);
    if (m > 0) HIPCHK(ctx, hipMemcpyAsync(d_x, dense, sizeof(float) * (size_t)m * words, hipMemcpyHostToDevice, ctx->stream));
    int32_t* d_p = S.upload(pos, (size_t)ns); NN(ctx, d_p);
    float* d_o = S.alloc<float>(no + 4); NN(ctx, d_o);
    HIPCHK(ctx, hipMemcpyAsync(d_o + skew_words, out, no * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    ScatterPlan plan;
    plan.add(d_x, d_o + skew_words, (size_t)words);
    slot_scatter_launch(plan, d_p, ns, ctx->stream);
    HIPCHK(ctx, hipMemcpyAsync(out, d_o + skew_words, no * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    return finish_op(ctx);
}

// ---- detection on a reduced frame: the per-op forms -------------------------------------------------------
static int downscale_impl(hp3d_ctx* ctx, const float* image, const uint8_t* image_u8, int B, int H, int W, int f, float* out) {
    if (!ctx) return HP3D_ERR_ARG;
    if ((!image && !image_u8) || !out || B < 1 || H < 1 || W < 1 || f < 1 || f > 8) HP3D_FAIL(ctx, HP3D_ERR_ARG, "bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Scratch S(ctx);
    const int Hd = (H + f - 1) / f, Wd = (W + f - 1) / f;
    const size_t ni = (size_t)B * H * W * 3, no = (size_t)B * Hd * Wd * 3;
    float* d_o = S.alloc<float>(no); NN(ctx, d_o);
    if (image_u8) {
        unsigned char* d_x = S.upload(image_u8, ni); NN(ctx, d_x);
        downscale_u8_launch(d_x, B, H, W, f, d_o, ctx->stream);
    } else {
        float* d_x = S.upload(image, ni); NN(ctx, d_x);
        downscale_launch(d_x, B, H, W, f, d_o, ctx->stream);
    }
    HIPCHK(ctx, hipMemcpyAsync(out, d_o, no * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    return finish_op(ctx);
}
int hp3d_downscale(hp3d_ctx* ctx, const float* image, int B, int H, int W, int f, float* out) {
    if (!ctx) return HP3D_ERR_ARG;
    if (!image) HP3D_FAIL(ctx, HP3D_ERR_ARG, "bad arguments");
    return downscale_impl(ctx, image, nullptr, B, H, W, f, out);
}
int hp3d_downscale_u8(hp3d_ctx* ctx, const uint8_t* image_u8, int B, int H, int W, int f, float* out) {
    if (!ctx) return HP3D_ERR_ARG;
    if (!image_u8) HP3D_FAIL(ctx, HP3D_ERR_ARG, "bad arguments");
    return downscale_impl(ctx, nullptr, image_u8, B, H, W, f, out);
}

// ---- detection on the lost frames only: the per-op form ---------------------------------------------------
int hp3d_gather_frames(hp3d_ctx* ctx, const float* image, const uint8_t* image_u8, int B, int H, int W, int f, const int32_t* idx, int m,
                       float* out) {
    if (!ctx) return HP3D_ERR_ARG;
    if ((image != nullptr) == (image_u8 != nullptr)) HP3D_FAIL(ctx, HP3D_ERR_ARG, "gather_frames: exactly one of image / image_u8");
    if (!idx || !out || B < 1 || H < 1 || W < 1 || f < 1 || f > 8) HP3D_FAIL(ctx, HP3D_ERR_ARG, "bad arguments");
    if (m < 1 || m > B) HP3D_FAIL(ctx, HP3D_ERR_ARG, "gather_frames: m = %d must be in 1 ... B = %d", m, B);
    for (int i = 0; i < m; ++i)
        if (idx[i] < 0 || idx[i] >= B || (i > 0 && idx[i] <= idx[i - 1]))
            HP3D_FAIL(ctx, HP3D_ERR_ARG, "gather_frames: idx[%d] = %d: idx must be strictly ascending in [0, %d)", i, (int)idx[i], B);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Scratch S(ctx);
    const int Hd = (H + f - 1) / f, Wd = (W + f - 1) / f;
    const size_t ni = (size_t)B * H * W * 3, no = (size_t)m * Hd * Wd * 3;
    float* d_o = S.alloc<float>(no); NN(ctx, d_o);
    int32_t* d_i = S.upload(idx, (size_t)m); NN(ctx, d_i);
    if (image_u8) {
        unsigned char* d_x = S.upload(image_u8, ni); NN(ctx, d_x);
        if (f > 1) downscale_u8_idx_launch(d_x, d_i, m, H, W, f, d_o, ctx->stream);
        else preprocess_u8_idx_launch(d_x, d_i, m, H, W, d_o, ctx->stream);
    } else {
        float* d_x = S.upload(image, ni); NN(ctx, d_x);
        if (f > 1) downscale_idx_launch(d_x, d_i, m, H, W, f, d_o, ctx->stream);
        else { frame_gather_launch(d_x, d_i, m, (size_t)H * W * 3, d_o, ctx->stream); ++ctx->frame_gather_launches; }
    }
    HIPCHK(ctx, hipMemcpyAsync(out, d_o, no * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    return finish_op(ctx);
}

// ---- the multi-hand tracker's detection on the frames that lost a hand only: the per-op forms ------------------
int hp3d_track_hands_partial_index(hp3d_ctx* ctx, int nb, int K, const int32_t* valid, const int32_t* lost, int32_t* idx, int32_t* pos,
                                   int32_t* m) {
    if (!ctx) return HP3D_ERR_ARG;
    if (!valid || !lost || !idx || !pos || !m || nb < 1) HP3D_FAIL(ctx, HP3D_ERR_ARG, "bad arguments");
    if (K < 1 || K > HP3D_MAX_HANDS) HP3D_FAIL(ctx, HP3D_ERR_ARG, "max hands K=%d must be in 1 ... %d", K, HP3D_MAX_HANDS);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Scratch S(ctx);
    const size_t ns = (size_t)nb * K;
    int32_t* d_v = S.upload(valid, ns); NN(ctx, d_v);
    int32_t* d_l = S.upload(lost, ns); NN(ctx, d_l);
    int32_t* d_i = S.alloc<int32_t>((size_t)nb); NN(ctx, d_i);
    int32_t* d_p = S.alloc<int32_t>((size_t)nb); NN(ctx, d_p);
    HIPCHK(ctx, hipMemsetAsync(d_i, 0xff, sizeof(int32_t) * (size_t)nb, ctx->stream));          // (the kernel writes idx[0 .. m) only: the rest reads -1)
    track_hands_partial_index_launch(d_v, d_l, nb, K, d_i, d_p, ctx->stream);
    HIPCHK(ctx, hipMemcpyAsync(idx, d_i, sizeof(int32_t) * (size_t)nb, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(pos, d_p, sizeof(int32_t) * (size_t)nb, hipMemcpyDeviceToHost, ctx->stream));
    CHK(finish_op(ctx));
    int n = 0;          // (from what the device wrote, not from the flags)
    while (n < nb && idx[n] >= 0) ++n;
    *m = n;
    return 0;
}

int hp3d_track_hands_select_pos(hp3d_ctx* ctx, int nb, int K, int m, const int32_t* pos, const int32_t* keep, const float* det_center,
                                const float* det_scale, const int32_t* det_valid, const int32_t* det_area, const int32_t* det_claimed,
                                float* box_center, float* box_scale, int32_t* valid, int32_t* detected, int32_t* area, int32_t* claimed) {
    if (!ctx) return HP3D_ERR_ARG;
    if (!pos || !keep || !box_center || !box_scale || !valid || !detected || !area || !claimed || nb < 1 || m < 0 || m > nb)
        HP3D_FAIL(ctx, HP3D_ERR_ARG, "bad arguments");
    if (m > 0 && (!det_center || !det_scale || !det_valid || !det_area || !det_claimed)) HP3D_FAIL(ctx, HP3D_ERR_ARG, "bad arguments");
    if (K < 1 || K > HP3D_MAX_HANDS) HP3D_FAIL(ctx, HP3D_ERR_ARG, "max hands K=%d must be in 1 ... %d", K, HP3D_MAX_HANDS);
    for (int b = 0; b < nb; ++b)
        if (pos[b] < -1 || pos[b] >= m) HP3D_FAIL(ctx, HP3D_ERR_ARG, "pos[%d] = %d is no dense index of %d", b, (int)pos[b], m);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Scratch S(ctx);
    const size_t ns = (size_t)nb * K, nd = (size_t)std::max(m, 1) * K;
    int32_t* d_p = S.upload(pos, (size_t)nb); NN(ctx, d_p);
    int32_t* d_k = S.upload(keep, ns); NN(ctx, d_k);
    float* d_dc = S.alloc<float>(nd * 2); NN(ctx, d_dc);
    float* d_ds = S.alloc<float>(nd); NN(ctx, d_ds);
    int32_t* d_dv = S.alloc<int32_t>(nd); NN(ctx, d_dv);
    int32_t* d_da = S.alloc<int32_t>(nd); NN(ctx, d_da);
    int32_t* d_dk = S.alloc<int32_t>(nd); NN(ctx, d_dk);
    if (m > 0) {
        const size_t md = (size_t)m * K;
        HIPCHK(ctx, hipMemcpyAsync(d_dc, det_center, sizeof(float) * md * 2, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(d_ds, det_scale, sizeof(float) * md, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(d_dv, det_valid, sizeof(int32_t) * md, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(d_da, det_area, sizeof(int32_t) * md, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(d_dk, det_claimed, sizeof(int32_t) * md, hipMemcpyHostToDevice, ctx->stream));
    }
    // box_center / box_scale / valid are read first: a slot that keeps them must get them back untouched
    float* d_c = S.upload(box_center, ns * 2); NN(ctx, d_c);
    float* d_s = S.upload(box_scale, ns); NN(ctx, d_s);
    int32_t* d_v = S.upload(valid, ns); NN(ctx, d_v);
    int32_t* d_d = S.alloc<int32_t>(ns); NN(ctx, d_d);
    int32_t* d_a = S.alloc<int32_t>(ns); NN(ctx, d_a);
    int32_t* d_cl = S.alloc<int32_t>(ns); NN(ctx, d_cl);
    track_hands_select_pos_launch(d_p, nb, K, d_k, d_dc, d_ds, d_dv, d_da, d_dk, d_c, d_s, d_v, d_d, d_a, d_cl, ctx->stream);
    HIPCHK(ctx, hipMemcpyAsync(box_center, d_c, sizeof(float) * ns * 2, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(box_scale, d_s, sizeof(float) * ns, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(valid, d_v, sizeof(int32_t) * ns, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(detected, d_d, sizeof(int32_t) * ns, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(area, d_a, sizeof(int32_t) * ns, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(claimed, d_cl, sizeof(int32_t) * ns, hipMemcpyDeviceToHost, ctx->stream));
    return finish_op(ctx);
}

// ---- NV12 frames: the per-op forms ---------------------------------------------------------------------------
// Host planes at the caller's pitch and stride -> the same layout on the device (the kernels run on the pitch they were given); only
// bytes [0, W) of a row are read on the host too: the rows are placed into a zeroed span that is then uploaded.
static int upload_nv12_as_is(hp3d_ctx* ctx, Scratch& S, int B, int H, int W, const Nv12Arg& a, Nv12Src* out) {
    const size_t stride = B > 1 ? (size_t)a.frame_stride : 0;
    const size_t span_y = stride * (B - 1) + (size_t)a.pitch * (H - 1) + W, span_c = stride * (B - 1) + (size_t)a.pitch * (H / 2 - 1) + W;
    std::vector<unsigned char>& h = ctx->h_nv12;
    h.assign(span_y + span_c, 0);
    for (int b = 0; b < B; ++b) {
        for (int r = 0; r < H; ++r) memcpy(&h[b * stride + (size_t)r * a.pitch], a.y + b * stride + (size_t)r * a.pitch, W);
        for (int r = 0; r < H / 2; ++r) memcpy(&h[span_y + b * stride + (size_t)r * a.pitch], a.uv + b * stride + (size_t)r * a.pitch, W);
    }
    unsigned char* d = S.upload(h.data(), h.size()); NN(ctx, d);
    *out = nv12_src(d, d + span_y, a.pitch, stride, ctx->nv12_matrix);
    return 0;
}
int hp3d_nv12_to_rgb(hp3d_ctx* ctx, const uint8_t* y, const uint8_t* uv, int B, int H, int W, int pitch, int64_t frame_stride, uint8_t* out) {
    if (!ctx) return HP3D_ERR_ARG;
    const Nv12Arg nv{y, uv, pitch, (long long)frame_stride};
    CHK(check_nv12(ctx, B, H, W, nv));
    if (!out) HP3D_FAIL(ctx, HP3D_ERR_ARG, "nv12_to_rgb: out is NULL");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Scratch S(ctx);
    Nv12Src src;
    CHK(upload_nv12_as_is(ctx, S, B, H, W, nv, &src));
    const size_t no = (size_t)B * H * W * 3;
    unsigned char* d_o = S.alloc<unsigned char>(no); NN(ctx, d_o);
    nv12_to_rgb_launch(src, B, H, W, d_o, ctx->stream);
    HIPCHK(ctx, hipMemcpyAsync(out, d_o, no, hipMemcpyDeviceToHost, ctx->stream));
    return finish_op(ctx);
}
int hp3d_crop_and_resize_nv12(hp3d_ctx* ctx, const uint8_t* y, const uint8_t* uv, int B, int H, int W, int pitch, int64_t frame_stride, int K,
                              const float* center, const float* scale, const int32_t* idx, int m, int crop_size, float* out) {
    if (!ctx) return HP3D_ERR_ARG;
    const Nv12Arg nv{y, uv, pitch, (long long)frame_stride};
    CHK(check_nv12(ctx, B, H, W, nv));
    if (!center || !scale || !out || K < 1 || K > HP3D_MAX_HANDS || crop_size < 1) HP3D_FAIL(ctx, HP3D_ERR_ARG, "crop_and_resize_nv12: bad arguments");
    if (idx && (m < 0 || m > B * K)) HP3D_FAIL(ctx, HP3D_ERR_ARG, "crop_and_resize_nv12: m = %d must be in 0 ... B K = %d", m, B * K);
    for (int i = 0; idx && i < m; ++i)
        if (idx[i] < 0 || idx[i] >= B * K) HP3D_FAIL(ctx, HP3D_ERR_ARG, "idx[%d] = %d is no slot of %d", i, (int)idx[i], B * K);
    const int n = idx ? m : B * K;
    if (n == 0) return 0;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Scratch S(ctx);
    Nv12Src src;
    CHK(upload_nv12_as_is(ctx, S, B, H, W, nv, &src));
    const size_t no = (size_t)n * crop_size * crop_size * 3;
    float* d_c = S.upload(center, (size_t)B * K * 2); NN(ctx, d_c);
    float* d_s = S.upload(scale, (size_t)B * K); NN(ctx, d_s);
    int32_t* d_i = nullptr;
    if (idx) { d_i = S.upload(idx, (size_t)m); NN(ctx, d_i); }
    float* d_o = S.alloc<float>(no); NN(ctx, d_o);
    crop_and_resize_nv12_launch(src, n, H, W, d_c, d_s, d_i, K, crop_size, d_o, ctx->stream);
    ++ctx->crop_nv12_launches;
    HIPCHK(ctx, hipMemcpyAsync(out, d_o, no * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    return finish_op(ctx);
}
int hp3d_downscale_nv12(hp3d_ctx* ctx, const uint8_t* y, const uint8_t* uv, int B, int H, int W, int pitch, int64_t frame_stride, int f,
                        const int32_t* idx, int m, float* out) {
    if (!ctx) return HP3D_ERR_ARG;
    const Nv12Arg nv{y, uv, pitch, (long long)frame_stride};
    CHK(check_nv12(ctx, B, H, W, nv));
    if (!out || f < 1 || f > 8) HP3D_FAIL(ctx, HP3D_ERR_ARG, "downscale_nv12: bad arguments (f = %d must be in 1 ... 8)", f);
    if (idx && (m < 1 || m > B)) HP3D_FAIL(ctx, HP3D_ERR_ARG, "downscale_nv12: m = %d must be in 1 ... B = %d", m, B);
    for (int i = 0; idx && i < m; ++i)
        if (idx[i] < 0 || idx[i] >= B) HP3D_FAIL(ctx, HP3D_ERR_ARG, "downscale_nv12: idx[%d] = %d is no frame of %d", i, (int)idx[i], B);
    const int n = idx ? m : B;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Scratch S(ctx);
    Nv12Src src;
    CHK(upload_nv12_as_is(ctx, S, B, H, W, nv, &src));
    const int Hd = (H + f - 1) / f, Wd = (W + f - 1) / f;
    const size_t no = (size_t)n * Hd * Wd * 3;
    int32_t* d_i = nullptr;
    if (idx) { d_i = S.upload(idx, (size_t)m); NN(ctx, d_i); }
    float* d_o = S.alloc<float>(no); NN(ctx, d_o);
    downscale_nv12_launch(src, d_i, n, H, W, f, d_o, ctx->stream);
    HIPCHK(ctx, hipMemcpyAsync(out, d_o, no * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    return finish_op(ctx);
}

// ---- packed 8-bit frames: the per-op forms ---------------------------------------------------------------------
// A host surface at the caller's pitch and stride -> the same layout on the device, at the caller's base misalignment (modulo 16), so
// that the kernels run on what they were given.  Only bytes [0, W pixel_bytes) of a row are read on the host: the rows are placed into
// a span of 255s that is then uploaded.
static int upload_px_as_is(hp3d_ctx* ctx, Scratch& S, int B, int H, int W, const PxArg& a, PxSrc* out) {
    const size_t stride = B > 1 ? (size_t)a.frame_stride : 0, row = (size_t)W * px_pixel_bytes(a.format);
    const size_t lead = (uintptr_t)a.px % 16, span = stride * (B - 1) + (size_t)a.pitch * (H - 1) + row;
    std::vector<unsigned char>& h = ctx->h_px;
    h.assign(lead + span, 255);
    for (int b = 0; b < B; ++b)
        for (int r = 0; r < H; ++r) memcpy(&h[lead + b * stride + (size_t)r * a.pitch], a.px + b * stride + (size_t)r * a.pitch, row);
    unsigned char* d = S.upload(h.data(), h.size()); NN(ctx, d);
    *out = px_src(d + lead, a.pitch, stride, a.format);
    return 0;
}
int hp3d_px_to_rgb(hp3d_ctx* ctx, const uint8_t* px, int B, int H, int W, int pitch, int64_t frame_stride, int format, uint8_t* out) {
    if (!ctx) return HP3D_ERR_ARG;
    const PxArg pa{px, pitch, (long long)frame_stride, format};
    CHK(check_px(ctx, B, H, W, pa));
    if (!out) HP3D_FAIL(ctx, HP3D_ERR_ARG, "px_to_rgb: out is NULL");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Scratch S(ctx);
    PxSrc src;
    CHK(upload_px_as_is(ctx, S, B, H, W, pa, &src));
    const size_t no = (size_t)B * H * W * 3;
    unsigned char* d_o = S.alloc<unsigned char>(no); NN(ctx, d_o);
    px_to_rgb_launch(src, B, H, W, d_o, ctx->stream);
    HIPCHK(ctx, hipMemcpyAsync(out, d_o, no, hipMemcpyDeviceToHost, ctx->stream));
    return finish_op(ctx);
}
int hp3d_crop_and_resize_px(hp3d_ctx* ctx, const uint8_t* px, int B, int H, int W, int pitch, int64_t frame_stride, int format, int K,
                            const float* center, const float* scale, const int32_t* idx, int m, int crop_size, float* out) {
    if (!ctx) return HP3D_ERR_ARG;
    const PxArg pa{px, pitch, (long long)frame_stride, format};
    CHK(check_px(ctx, B, H, W, pa));
    if (!center || !scale || !out || K < 1 || K > HP3D_MAX_HANDS || crop_size < 1) HP3D_FAIL(ctx, HP3D_ERR_ARG, "crop_and_resize_px: bad arguments");
    if (idx && (m < 0 || m > B * K)) HP3D_FAIL(ctx, HP3D_ERR_ARG, "crop_and_resize_px: m = %d must be in 0 ... B K = %d", m, B * K);
    for (int i = 0; idx && i < m; ++i)
        if (idx[i] < 0 || idx[i] >= B * K) HP3D_FAIL(ctx, HP3D_ERR_ARG, "idx[%d] = %d is no slot of %d", i, (int)idx[i], B * K);
    const int n = idx ? m : B * K;
    if (n == 0) return 0;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Scratch S(ctx);
    PxSrc src;
    CHK(upload_px_as_is(ctx, S, B, H, W, pa, &src));
    const size_t no = (size_t)n * crop_size * crop_size * 3;
    float* d_c = S.upload(center, (size_t)B * K * 2); NN(ctx, d_c);
    float* d_s = S.upload(scale, (size_t)B * K); NN(ctx, d_s);
    int32_t* d_i = nullptr;
    if (idx) { d_i = S.upload(idx, (size_t)m); NN(ctx, d_i); }
    float* d_o = S.alloc<float>(no); NN(ctx, d_o);
    crop_and_resize_px_launch(src, n, H, W, d_c, d_s, d_i, K, crop_size, d_o, ctx->stream);
    ++ctx->crop_px_launches;
    HIPCHK(ctx, hipMemcpyAsync(out, d_o, no * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    return finish_op(ctx);
}
int hp3d_downscale_px(hp3d_ctx* ctx, const uint8_t* px, int B, int H, int W, int pitch, int64_t frame_stride, int format, int f,
                      const int32_t* idx, int m, float* out) {
    if (!ctx) return HP3D_ERR_ARG;
    const PxArg pa{px, pitch, (long long)frame_stride, format};
    CHK(check_px(ctx, B, H, W, pa));
    if (!out || f < 1 || f > 8) HP3D_FAIL(ctx, HP3D_ERR_ARG, "downscale_px: bad arguments (f = %d must be in 1 ... 8)", f);
    if (idx && (m < 1 || m > B)) HP3D_FAIL(ctx, HP3D_ERR_ARG, "downscale_px: m = %d must be in 1 ... B = %d", m, B);
    for (int i = 0; idx && i < m; ++i)
        if (idx[i] < 0 || idx[i] >= B) HP3D_FAIL(ctx, HP3D_ERR_ARG, "downscale_px: idx[%d] = %d is no frame of %d", i, (int)idx[i], B);
    const int n = idx ? m : B;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Scratch S(ctx);
    PxSrc src;
    CHK(upload_px_as_is(ctx, S, B, H, W, pa, &src));
    const int Hd = (H + f - 1) / f, Wd = (W + f - 1) / f;
    const size_t no = (size_t)n * Hd * Wd * 3;
    int32_t* d_i = nullptr;
    if (idx) { d_i = S.upload(idx, (size_t)m); NN(ctx, d_i); }
    float* d_o = S.alloc<float>(no); NN(ctx, d_o);
    downscale_px_launch(src, d_i, n, H, W, f, d_o, ctx->stream);
    HIPCHK(ctx, hipMemcpyAsync(out, d_o, no * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    return finish_op(ctx);
}

// ---- a batch of separate surfaces: the per-op forms -----------------------------------------------------------------
// Every host surface -> an allocation of its own on the device (NV12: one per plane), at the caller's pitch and base misalignment
// (modulo 16), so that the kernels run on what they were given and every surface decides its own wide paths.  Only the picture's bytes
// of a row are read on the host: the rows are placed into spans of 255s that are then uploaded.
static int upload_surf_as_is(hp3d_ctx* ctx, Scratch& S, int B, int H, int W, const hp3d_surface* sf, SurfSrc* out) {
    // plane p of surface b: rows[p] rows of `row` bytes at the surface's pitch
    auto planes = [&](const hp3d_surface& s, const unsigned char** base, int* rows) {
        base[0] = s.data; rows[0] = H;
        base[1] = s.chroma; rows[1] = H / 2;
        return s.format == HP3D_SURF_NV12 ? 2 : 1;
    };
    size_t total = 0;
    for (int b = 0; b < B; ++b) {
        const unsigned char* base[2]; int rows[2];
        const int np = planes(sf[b], base, rows);
        for (int p = 0; p < np; ++p) total += (uintptr_t)base[p] % 16 + (size_t)sf[b].pitch * (rows[p] - 1) + surf_row_bytes(sf[b], W);
    }
    std::vector<unsigned char>& h = ctx->h_px;
    h.assign(total, 255);
    SurfRec* rec;
    CHK(surf_table_begin(ctx, B, &rec));
    size_t at = 0;
    for (int b = 0; b < B; ++b) {
        const hp3d_surface& s = sf[b];
        const size_t row = surf_row_bytes(s, W);
        const unsigned char* base[2]; int rows[2];
        const int np = planes(s, base, rows);
        const unsigned char* d_plane[2] = {nullptr, nullptr};
        for (int p = 0; p < np; ++p) {
            const size_t lead = (uintptr_t)base[p] % 16, span = lead + (size_t)s.pitch * (rows[p] - 1) + row;
            for (int r = 0; r < rows[p]; ++r) memcpy(&h[at + lead + (size_t)r * s.pitch], base[p] + (size_t)r * s.pitch, row);
            unsigned char* d = S.upload(&h[at], span); NN(ctx, d);
            d_plane[p] = d + lead;
            at += span;
        }
        rec[b] = surf_rec(d_plane[0], d_plane[1], s.pitch, s.format);
    }
    return surf_table_commit(ctx, B, out);
}
int hp3d_surf_to_rgb(hp3d_ctx* ctx, const hp3d_surface* surfaces, int B, int H, int W, uint8_t* out) {
    if (!ctx) return HP3D_ERR_ARG;
    CHK(check_surfaces(ctx, B, H, W, surfaces));
    if (!out) HP3D_FAIL(ctx, HP3D_ERR_ARG, "surf_to_rgb: out is NULL");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Scratch S(ctx);
    SurfSrc src;
    CHK(upload_surf_as_is(ctx, S, B, H, W, surfaces, &src));
    const size_t no = (size_t)B * H * W * 3;
    unsigned char* d_o = S.alloc<unsigned char>(no); NN(ctx, d_o);
    surf_to_rgb_launch(src, B, H, W, d_o, ctx->stream);
    HIPCHK(ctx, hipMemcpyAsync(out, d_o, no, hipMemcpyDeviceToHost, ctx->stream));
    return finish_op(ctx);
}
int hp3d_crop_and_resize_surf(hp3d_ctx* ctx, const hp3d_surface* surfaces, int B, int H, int W, int K, const float* center,
                              const float* scale, const int32_t* idx, int m, int crop_size, float* out) {
    if (!ctx) return HP3D_ERR_ARG;
    CHK(check_surfaces(ctx, B, H, W, surfaces));
    if (!center || !scale || !out || K < 1 || K > HP3D_MAX_HANDS || crop_size < 1) HP3D_FAIL(ctx, HP3D_ERR_ARG, "crop_and_resize_surf: bad arguments");
    if (idx && (m < 0 || m > B * K)) HP3D_FAIL(ctx, HP3D_ERR_ARG, "crop_and_resize_surf: m = %d must be in 0 ... B K = %d", m, B * K);
    for (int i = 0; idx && i < m; ++i)
        if (idx[i] < 0 || idx[i] >= B * K) HP3D_FAIL(ctx, HP3D_ERR_ARG, "idx[%d] = %d is no slot of %d", i, (int)idx[i], B * K);
    const int n = idx ? m : B * K;
    if (n == 0) return 0;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Scratch S(ctx);
    SurfSrc src;
    CHK(upload_surf_as_is(ctx, S, B, H, W, surfaces, &src));
    const size_t no = (size_t)n * crop_size * crop_size * 3;
    float* d_c = S.upload(center, (size_t)B * K * 2); NN(ctx, d_c);
    float* d_s = S.upload(scale, (size_t)B * K); NN(ctx, d_s);
    int32_t* d_i = nullptr;
    if (idx) { d_i = S.upload(idx, (size_t)m); NN(ctx, d_i); }
    float* d_o = S.alloc<float>(no); NN(ctx, d_o);
    crop_and_resize_surf_launch(src, n, H, W, d_c, d_s, d_i, K, crop_size, d_o, ctx->stream);
    ++ctx->crop_surf_launches;
    HIPCHK(ctx, hipMemcpyAsync(out, d_o, no * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    return finish_op(ctx);
}
int hp3d_downscale_surf(hp3d_ctx* ctx, const hp3d_surface* surfaces, int B, int H, int W, int f, const int32_t* idx, int m, float* out) {
    if (!ctx) return HP3D_ERR_ARG;
    CHK(check_surfaces(ctx, B, H, W, surfaces));
    if (!out || f < 1 || f > 8) HP3D_FAIL(ctx, HP3D_ERR_ARG, "downscale_surf: bad arguments (f = %d must be in 1 ... 8)", f);
    if (idx && (m < 1 || m > B)) HP3D_FAIL(ctx, HP3D_ERR_ARG, "downscale_surf: m = %d must be in 1 ... B = %d", m, B);
    for (int i = 0; idx && i < m; ++i)
        if (idx[i] < 0 || idx[i] >= B) HP3D_FAIL(ctx, HP3D_ERR_ARG, "downscale_surf: idx[%d] = %d is no frame of %d", i, (int)idx[i], B);
    const int n = idx ? m : B;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Scratch S(ctx);
    SurfSrc src;
    CHK(upload_surf_as_is(ctx, S, B, H, W, surfaces, &src));
    const int Hd = (H + f - 1) / f, Wd = (W + f - 1) / f;
    const size_t no = (size_t)n * Hd * Wd * 3;
    int32_t* d_i = nullptr;
    if (idx) { d_i = S.upload(idx, (size_t)m); NN(ctx, d_i); }
    float* d_o = S.alloc<float>(no); NN(ctx, d_o);
    downscale_surf_launch(src, d_i, n, H, W, f, d_o, ctx->stream);
    HIPCHK(ctx, hipMemcpyAsync(out, d_o, no * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    return finish_op(ctx);
}

int hp3d_boxes_to_frame(hp3d_ctx* ctx, int n, int f, const float* center_d, const float* crop_size_d, float* center, float* crop_size,
                        float* scale) {
    if (!ctx) return HP3D_ERR_ARG;
    if (!center_d || !crop_size_d || !center || !crop_size || !scale || n < 1 || f < 1 || f > 8) HP3D_FAIL(ctx, HP3D_ERR_ARG, "bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Scratch S(ctx);
    float* d_c = S.upload(center_d, (size_t)n * 2); NN(ctx, d_c);
    float* d_cs = S.upload(crop_size_d, (size_t)n); NN(ctx, d_cs);
    float* d_s = S.alloc<float>(n); NN(ctx, d_s);
    box_to_frame_launch(d_c, d_cs, n, f, d_c, d_cs, d_s, ctx->stream);          // in place, as the step runs it
    HIPCHK(ctx, hipMemcpyAsync(center, d_c, sizeof(float) * (size_t)n * 2, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(crop_size, d_cs, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(scale, d_s, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    return finish_op(ctx);
}

int hp3d_boxes_to_detect(hp3d_ctx* ctx, int n, int f, const float* center, const float* scale, float* center_d, float* scale_d) {
    if (!ctx) return HP3D_ERR_ARG;
    if (!center || !scale || !center_d || !scale_d || n < 1 || f < 1 || f > 8) HP3D_FAIL(ctx, HP3D_ERR_ARG, "bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Scratch S(ctx);
    float* d_c = S.upload(center, (size_t)n * 2); NN(ctx, d_c);
    float* d_s = S.upload(scale, (size_t)n); NN(ctx, d_s);
    float* d_cd = S.alloc<float>((size_t)n * 2); NN(ctx, d_cd);
    float* d_sd = S.alloc<float>(n); NN(ctx, d_sd);
    box_to_detect_launch(d_c, d_s, n, f, d_cd, d_sd, ctx->stream);
    HIPCHK(ctx, hipMemcpyAsync(center_d, d_cd, sizeof(float) * (size_t)n * 2, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(scale_d, d_sd, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    return finish_op(ctx);
}

int hp3d_preprocess_u8(hp3d_ctx* ctx, const uint8_t* image_u8, int B, int Hin, int Win, int H, int W, float* out) {
    if (!ctx) return HP3D_ERR_ARG;
    if (!image_u8 || !out || B < 1 || Hin < 2 || Win < 2 || H < 1 || W < 1) HP3D_FAIL(ctx, HP3D_ERR_ARG, "bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Scratch S(ctx);
    unsigned char* d_in = S.upload(image_u8, (size_t)B * Hin * Win * 3); NN(ctx, d_in);
    float* d_o = S.alloc<float>((size_t)B * H * W * 3); NN(ctx, d_o);
    preprocess_u8_launch(d_in, B, Hin, Win, H, W, d_o, ctx->stream);
    HIPCHK(ctx, hipMemcpyAsync(out, d_o, sizeof(float) * (size_t)B * H * W * 3, hipMemcpyDeviceToHost, ctx->stream));
    return finish_op(ctx);
}

int hp3d_infer_2d_kp(hp3d_ctx* ctx, int B, int H, int W, const float* image, float* keypoints_scoremap,
                     float* image_crop, float* scale_crop, float* center, int32_t* keypoint_hw_crop, double* keypoint_hw) {
    if (!ctx) return HP3D_ERR_ARG;
    if (!image) HP3D_FAIL(ctx, HP3D_ERR_ARG, "image is NULL");
    CHK(check_img(ctx, B, H, W));
    CHK(need_nets(ctx, NET_SEG | NET_POSE));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // same chunking as the full path (the float32 Winograd kernels address a chunk with 32-bit offsets)
    const int mb0 = auto_micro_batch(ctx, B, H, W);
    const int mb = mb0 <= 0 ? B : std::min(mb0, B);
    CHK(ensure_arena(ctx, mb, H, W));
    const int saved_prof = ctx->profiling;
    struct ProfRestore { hp3d_ctx* c; int v; ~ProfRestore() { c->profiling = v; } } prof_restore{ctx, saved_prof};   // every exit path
    if (ctx->profiling != 2) prof_reset(ctx);   // mode 2 accumulates across calls
    for (int b0 = 0; b0 < B; b0 += mb) {
        const int nb = std::min(mb, B - b0);
        if (b0 > 0 && saved_prof == 1) ctx->profiling = 2;
        CHK(copy_in(ctx, ctx->d_image, image + (size_t)b0 * H * W * 3, (size_t)nb * H * W * 3, false));
        CHK(run_detect_and_crop(ctx, ctx->d_image, nb, H, W, 0));
        CHK(run_posenet(ctx, ctx->d_crop, nb, 256, 256, true));
        if (keypoints_scoremap) {
            resize_bilinear_launch(ctx->d_sm[2], nb, 32, 32, 21, 32, 256, 256, ctx->d_kpmap, ctx->stream);
            CHK(copy_out(ctx, keypoints_scoremap + (size_t)b0 * 256 * 256 * 21, ctx->d_kpmap, (size_t)nb * 256 * 256 * 21, false));
        }
        if (keypoint_hw_crop || keypoint_hw)
            CHK(run_kp_detect(ctx, nb, keypoint_hw_crop ? keypoint_hw_crop + (size_t)b0 * 42 : nullptr,
                              keypoint_hw ? keypoint_hw + (size_t)b0 * 42 : nullptr, false));
        if (image_crop) CHK(copy_out(ctx, image_crop + (size_t)b0 * 256 * 256 * 3, ctx->d_crop, (size_t)nb * 256 * 256 * 3, false));
        if (scale_crop) CHK(copy_out(ctx, scale_crop + b0, ctx->d_scale, (size_t)nb, false));
        if (center) CHK(copy_out(ctx, center + (size_t)b0 * 2, ctx->d_center, (size_t)nb * 2, false));
    }
    return finish_op(ctx);
}
int hp3d_infer_2d(hp3d_ctx* ctx, int B, int H, int W, const float* image, float* keypoints_scoremap,
                  float* image_crop, float* scale_crop, float* center) {
    return hp3d_infer_2d_kp(ctx, B, H, W, image, keypoints_scoremap, image_crop, scale_crop, center, nullptr, nullptr);
}

// hp3d_detect_keypoints: detect_keypoints(tf.image.resize_images(scoremap, (oh, ow))) per image and channel without the
// large map (utils/general.py:331-344 on the output of CHP3D.py:97); scoremap [B,h,w,C] with h*w <= 4096
int hp3d_detect_keypoints(hp3d_ctx* ctx, const float* scoremap, int B, int h, int w, int C, int oh, int ow, int32_t* out_rc) {
    if (!ctx) return HP3D_ERR_ARG;
    if (!scoremap || !out_rc || B < 1 || h < 1 || w < 1 || C < 1 || oh < 1 || ow < 1 || h * w > 4096)
        HP3D_FAIL(ctx, HP3D_ERR_ARG, "bad arguments (h*w must be <= 4096)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Scratch S(ctx);
    float* d_x = S.upload(scoremap, (size_t)B * h * w * C); NN(ctx, d_x);
    int* d_o = S.alloc<int>((size_t)B * C * 2); NN(ctx, d_o);
    kp_detect_launch(d_x, B, h, w, C, C, oh, ow, nullptr, nullptr, d_o, nullptr, ctx->stream);
    HIPCHK(ctx, hipMemcpyAsync(out_rc, d_o, sizeof(int) * (size_t)B * C * 2, hipMemcpyDeviceToHost, ctx->stream));
    return finish_op(ctx);
}

int hp3d_handsegnet(hp3d_ctx* ctx, int B, int H, int W, const float* image, float* scoremap_large,
                    float* scoremap_small) {
    if (!ctx) return HP3D_ERR_ARG;
    if (!image) HP3D_FAIL(ctx, HP3D_ERR_ARG, "image is NULL");
    CHK(check_img(ctx, B, H, W));
    CHK(need_nets(ctx, NET_SEG));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    CHK(ensure_arena(ctx, B, H, W));
    if (ctx->profiling != 2) prof_reset(ctx);   // mode 2 accumulates across calls
    CHK(copy_in(ctx, ctx->d_image, image, (size_t)B * H * W * 3, false));
    CHK(run_handsegnet(ctx, ctx->d_image, B, H, W));
    if (scoremap_large) {
        resize_bilinear_launch(ctx->d_segsmall, B, H / 8, W / 8, 2, 32, H, W, ctx->d_large, ctx->stream);
        CHK(copy_out(ctx, scoremap_large, ctx->d_large, (size_t)B * H * W * 2, false));
    }
    if (scoremap_small) {
        const int npix = B * (H / 8) * (W / 8);
        copy_channels_launch(ctx->d_segsmall, npix, 2, 32, ctx->bufA, 2, ctx->stream);
        CHK(copy_out(ctx, scoremap_small, ctx->bufA, (size_t)npix * 2, false));
    }
    return finish_op(ctx);
}

int hp3d_posenet2d(hp3d_ctx* ctx, int B, int H, int W, const float* image_crop, float* s0, float* s1, float* s2) {
    return posenet_impl(ctx, B, H, W, image_crop, s0, s1, s2, false);
}
int hp3d_posenet2d_dev(hp3d_ctx* ctx, int B, int H, int W, const float* image_crop, float* s0, float* s1, float* s2) {
    if (!ctx) return HP3D_ERR_ARG;
    return run_graphed(ctx, graph_key("posenet", {B, H, W}, {image_crop, s0, s1, s2}),
                       [&]() { return posenet_impl(ctx, B, H, W, image_crop, s0, s1, s2, true); });
}

static int lift_common(hp3d_ctx* ctx, int B, int variant, const float* d_sm32pad, const float* hand_side,
                       float* rel, float* can, float* rot) {
    CHK(copy_in(ctx, ctx->d_hs, hand_side, (size_t)B * 2, false));
    CHK(run_pose3d(ctx, d_sm32pad, ctx->d_hs, B, variant));
    CHK(copy_out(ctx, rel, ctx->d_coord, (size_t)B * 63, false));
    CHK(copy_out(ctx, can, ctx->d_can, (size_t)B * 63, false));
    if (variant == HP3D_VARIANT_PROPOSED) CHK(copy_out(ctx, rot, ctx->d_rot, (size_t)B * 9, false));
    return finish_op(ctx);
}

int hp3d_poseprior(hp3d_ctx* ctx, int B, int variant, const float* scoremap256, const float* hand_side,
                   float* coord_xyz_rel_normed, float* coord3d, float* rot_mat) {
    if (!ctx) return HP3D_ERR_ARG;
    if (!scoremap256 || !hand_side || B < 1) HP3D_FAIL(ctx, HP3D_ERR_ARG, "bad arguments");
    if (variant < 0 || variant > 3) HP3D_FAIL(ctx, HP3D_ERR_ARG, "Unknown variant.");
    CHK(need_nets(ctx, variant == HP3D_VARIANT_PROPOSED ? (NET_PRIOR | NET_VP)
                       : variant == HP3D_VARIANT_BOTTLENECK ? (NET_PRIOR | NET_BOTTLENECK) : NET_PRIOR));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    CHK(ensure_arena(ctx, B, 256, 256));
    if (ctx->profiling != 2) prof_reset(ctx);   // mode 2 accumulates across calls
    // stage the [B,256,256,21] GT scoremaps in bufA, pool 8x8 into the padded [B,32,32,32] buffer
    CHK(copy_in(ctx, ctx->bufB, scoremap256, (size_t)B * 256 * 256 * 21, false));
    HIPCHK(ctx, hipMemsetAsync(ctx->d_pooled, 0, sizeof(float) * (size_t)B * 32 * 32 * 32, ctx->stream));
    avgpool8_launch(ctx->bufB, B, 256, 256, 21, ctx->d_pooled, 32, ctx->stream);
    // the lifting convs ping-pong through bufA/bufB; d_pooled is separate
    return lift_common(ctx, B, variant, ctx->d_pooled, hand_side, coord_xyz_rel_normed, coord3d, rot_mat);
}

int hp3d_pose3d(hp3d_ctx* ctx, int B, const float* scoremap32, const float* hand_side, float* coord_xyz_rel_normed,
                float* coord_can, float* rot_mat) {
    if (!ctx) return HP3D_ERR_ARG;
    if (!scoremap32 || !hand_side || B < 1) HP3D_FAIL(ctx, HP3D_ERR_ARG, "bad arguments");
    CHK(need_nets(ctx, NET_PRIOR | NET_VP));
    HIPCHK(ctx, hipSetDevice(ctx->device));
    CHK(ensure_arena(ctx, B, 256, 256));
    if (ctx->profiling != 2) prof_reset(ctx);   // mode 2 accumulates across calls
    CHK(copy_in(ctx, ctx->bufB, scoremap32, (size_t)B * 32 * 32 * 21, false));
    pad_channels_launch(ctx->bufB, B * 32 * 32, 21, ctx->d_pooled, 32, ctx->stream);
    return lift_common(ctx, B, HP3D_VARIANT_PROPOSED, ctx->d_pooled, hand_side, coord_xyz_rel_normed, coord_can, rot_mat);
}

// ---- per-op entry points -----------------------------------------------------------------------
int hp3d_conv2d(hp3d_ctx* ctx, const float* x, int B, int H, int W, int Cin, const float* w_hwio, const float* bias,
                int k, int stride, int Cout, int act, int pool, float* out) {
    if (!ctx) return HP3D_ERR_ARG;
    if (!x || !w_hwio || !bias || !out || B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1)
        HP3D_FAIL(ctx, HP3D_ERR_ARG, "bad arguments");
    if (ctx->conv_naive && pool) HP3D_FAIL(ctx, HP3D_ERR_UNSUPPORTED, "naive conv has no fused pool");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (ctx->profiling != 2) prof_reset(ctx);
    ConvL l;
    l.name = "op/conv2d";
    l.k = k; l.cin = Cin; l.cout = Cout; l.stride = stride; l.relu = act; l.net = 0;
    // the conv1_1 shape (nets/ColorHandPose3DNetwork.py:144,183) runs as the networks' first layer (32 x 64 im2col filters, conv_first.hip);
    // every other Cin = 3 layer as a plain one: the im2col form sums in another order
    l.mode = k == 3 && Cin == 3 && Cout == 64 && !pool && ctx->use_first && ctx->use_wino != 2 && conv_first_eligible(k, stride, Cin, Cout, B, H, W, Cout, 0);
    l.ek = l.mode ? 1 : k; l.cin_pad = pad32(Cin); l.cout_pad = pad32(Cout);
    // The Winograd sections are the op's selection rule (pick_wino takes a form whose section exists): a form whose option is forced
    // to "1", else F(2x2,3x3) where conv_wino_eligible allows -- no cost model -- and all of them for Cout % 64 == 0 only.
    int secs = 0;
    if (ctx->use_wino && !l.mode && (k == 3 || k == 7) && stride == 1) {
        if (ctx->use_wino == 2) {       // conv_impl=winograd: no silent fallback
            l.cin_pad = (Cin + 63) / 64 * 64;
            if (Cout % 64) HP3D_FAIL(ctx, HP3D_ERR_UNSUPPORTED, "conv_impl=winograd needs Cout %% 64 == 0 (got %d)", Cout);
        }
        if (Cout % 64 == 0)
            secs = SEC_WINO | (ctx->use_wino2 == 1 ? SEC_WINO2 : 0) | (ctx->use_wino4 == 1 ? SEC_WINO4 : 0) |
                   (ctx->use_wino4s == 1 && k == 3 ? SEC_WINO4S : 0) | (ctx->use_wino7 == 1 && k == 7 ? SEC_WINO7 : 0);
    }
    size_t floats = 0, halves = 0;
    reserve_conv(l, secs, floats, halves);
    std::vector<float> packed(floats, 0.f);
    pack_layer(l, w_hwio, bias, packed.data());
    const int in_cs = l.mode ? Cin : l.cin_pad;
    Scratch S(ctx);
    float* d_pk = S.upload(packed.data(), packed.size()); NN(ctx, d_pk);
    float* d_w = nullptr;
    if (ctx->conv_naive) { d_w = S.upload(w_hwio, (size_t)k * k * Cin * Cout); NN(ctx, d_w); }
    float* d_x = S.upload(x, (size_t)B * H * W * Cin); NN(ctx, d_x);
    if (in_cs != Cin) {
        float* d_xp = S.alloc<float>((size_t)B * H * W * in_cs); NN(ctx, d_xp);
        pad_channels_launch(d_x, B * H * W, Cin, d_xp, in_cs, ctx->stream);
        d_x = d_xp;
    }
    int Ho, Wo, pad;
    same_pad(H, k, stride, &Ho, &pad);
    same_pad(W, k, stride, &Wo, &pad);
    const size_t out_floats = (size_t)B * (pool ? Ho / 2 : Ho) * (pool ? Wo / 2 : Wo) * Cout;
    float* d_out = S.alloc<float>(out_floats); NN(ctx, d_out);
    CHK(run_conv(ctx, ConvW{d_pk, nullptr, d_w}, l, d_x, in_cs, B, H, W, d_out, Cout, pool, nullptr, nullptr));
    HIPCHK(ctx, hipMemcpyAsync(out, d_out, sizeof(float) * out_floats, hipMemcpyDeviceToHost, ctx->stream));
    return finish_op(ctx);
}

// The half-precision per-op entry points hand float32 back: a device result [n, cs] of halves (or float32: an out_f32 head) comes to
// the host whole and its channels 0 .. C-1 are widened there (exact).  Ends the call like finish_op.
static int finish_op_f16(hp3d_ctx* ctx, const void* d_out, size_t n, int cs, int C, int is_f32, float* out) {
    std::vector<char> host(n * cs * (is_f32 ? 4 : 2));
    HIPCHK(ctx, hipMemcpyAsync(host.data(), d_out, host.size(), hipMemcpyDeviceToHost, ctx->stream));
    CHK(finish_op(ctx));
    const float* hf = (const float*)host.data();
    const hp3d_f16* hh = (const hp3d_f16*)host.data();
    for (size_t i = 0; i < n; ++i)
        for (int c = 0; c < C; ++c) out[i * C + c] = is_f32 ? hf[i * cs + c] : (float)hh[i * cs + c];
    return 0;
}

// One layer of a half-precision trunk ("op/conv2d_f16"): built and run like hp3d_conv2d's, through run_conv(f16 = 1).  The layer is
// a plain one (mode 0) or the networks' first (mode 1: the raw float32 image); the concat permutation of mode 2 is a network matter.
int hp3d_conv2d_f16(hp3d_ctx* ctx, const float* x, int B, int H, int W, int Cin, const float* w_hwio, const float* bias,
                    int k, int stride, int Cout, int act, int pool, int out_f32, float* out) {
    if (!ctx) return HP3D_ERR_ARG;
    if (!x || !w_hwio || !bias || !out || B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || k < 1 || stride < 1 || (long)B * H * W > 0x7fffffffL)
        HP3D_FAIL(ctx, HP3D_ERR_ARG, "bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (ctx->profiling != 2) prof_reset(ctx);
    ConvL l;
    l.name = "op/conv2d_f16";
    l.k = k; l.cin = Cin; l.cout = Cout; l.stride = stride; l.relu = act; l.net = 0;
    l.mode = k == 3 && stride == 1 && Cin == 3 && Cout == 64 && !pool && !out_f32;       // the conv1_1 shape, as Tables::add_conv lays it out
    l.ek = l.mode ? 1 : k; l.cin_pad = pad32(Cin); l.cout_pad = pad32(Cout);
    size_t floats = 0, halves = 0;
    reserve_conv(l, SEC_F16, floats, halves);
    std::vector<float> packed(floats, 0.f);
    pack_layer(l, w_hwio, bias, packed.data());            // the bias and conv1_1's im2col filter
    std::vector<hp3d_f16> packed16(halves);
    pack_conv16(l, w_hwio, packed16.data());
    const size_t npix = (size_t)B * H * W;
    Scratch S(ctx);
    float* d_pk = S.upload(packed.data(), packed.size()); NN(ctx, d_pk);
    hp3d_f16* d_pk16 = S.upload(packed16.data(), packed16.size()); NN(ctx, d_pk16);
    float* d_x = S.upload(x, npix * Cin); NN(ctx, d_x);
    const float* d_in = d_x;
    int in_cs = Cin;
    if (!l.mode) {         // what a trunk layer is fed: halves, channel stride cin_pad16, zero padding
        hp3d_f16* d_x16 = S.alloc<hp3d_f16>(npix * l.cin_pad16); NN(ctx, d_x16);
        HIPCHK(ctx, hipMemsetAsync(d_x16, 0, npix * l.cin_pad16 * sizeof(hp3d_f16), ctx->stream));
        cvt_channels_f16_launch(d_x, (int)npix, Cin, Cin, d_x16, l.cin_pad16, ctx->stream);
        d_in = (const float*)d_x16; in_cs = l.cin_pad16;
    }
    int Ho, Wo, pad;
    same_pad(H, l.ek, stride, &Ho, &pad);
    same_pad(W, l.ek, stride, &Wo, &pad);
    const size_t opix = (size_t)B * (pool ? Ho / 2 : Ho) * (pool ? Wo / 2 : Wo);
    const int out_cs = l.cout_pad;
    const size_t obytes = opix * out_cs * (out_f32 ? 4 : 2);
    char* d_out = S.alloc<char>(obytes); NN(ctx, d_out);
    HIPCHK(ctx, hipMemsetAsync(d_out, 0xff, obytes, ctx->stream));        // (an output no kernel stores comes back as NaN)
    CHK(run_conv(ctx, ConvW{d_pk, d_pk16, nullptr}, l, d_in, in_cs, B, H, W, (float*)d_out, out_cs, pool, nullptr, nullptr, 1, out_f32));
    return finish_op_f16(ctx, d_out, opix, out_cs, Cout, out_f32, out);
}

// The first block of a half-precision trunk (conv1_1 + conv1_2 + 2x2 max-pool) as run_trunk runs it: the fused launch where option
// "f16_fuse12" and the shape allow, else conv1_1 and the pooled conv1_2 one by one.
int hp3d_first_block_f16(hp3d_ctx* ctx, const float* image, int B, int H, int W, const float* w1, const float* b1, const float* w2,
                         const float* b2, float* out) {
    if (!ctx) return HP3D_ERR_ARG;
    if (!image || !w1 || !b1 || !w2 || !b2 || !out || B < 1 || H < 2 || W < 2 || (long)B * H * W > 0x7fffffffL) HP3D_FAIL(ctx, HP3D_ERR_ARG, "bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (ctx->profiling != 2) prof_reset(ctx);
    ConvL l1, l2;
    l1.name = "op/first_block_f16/conv1_1"; l2.name = "op/first_block_f16/conv1_2";
    l1.k = l2.k = 3; l1.cin = 3; l2.cin = 64; l1.cout = l2.cout = 64; l1.stride = l2.stride = 1; l1.relu = l2.relu = 1; l1.net = l2.net = 0;
    l1.mode = 1; l1.ek = 1; l1.cin_pad = 32; l1.cout_pad = 64;
    l2.mode = 0; l2.ek = 3; l2.cin_pad = 64; l2.cout_pad = 64;
    size_t floats = 0, halves = 0;
    reserve_conv(l1, SEC_F16, floats, halves);
    reserve_conv(l2, SEC_F16, floats, halves);
    std::vector<float> packed(floats, 0.f);
    std::vector<hp3d_f16> packed16(halves);
    pack_layer(l1, w1, b1, packed.data());
    pack_layer(l2, w2, b2, packed.data());
    pack_conv16(l1, w1, packed16.data());
    pack_conv16(l2, w2, packed16.data());
    const size_t npix = (size_t)B * H * W, opix = (size_t)B * (H / 2) * (W / 2);
    Scratch S(ctx);
    float* d_pk = S.upload(packed.data(), packed.size()); NN(ctx, d_pk);
    hp3d_f16* d_pk16 = S.upload(packed16.data(), packed16.size()); NN(ctx, d_pk16);
    float* d_img = S.upload(image, npix * 3); NN(ctx, d_img);
    hp3d_f16* d_out = S.alloc<hp3d_f16>(opix * 64); NN(ctx, d_out);
    HIPCHK(ctx, hipMemsetAsync(d_out, 0xff, opix * 64 * sizeof(hp3d_f16), ctx->stream));
    const ConvW wts{d_pk, d_pk16, nullptr};
    int oh = 0, ow = 0;
    const int fused = run_fused12(ctx, wts, 1, l1, l2, d_img, B, H, W, (float*)d_out, &oh, &ow);
    if (fused < 0) return fused;
    if (!fused) {
        hp3d_f16* d_a = S.alloc<hp3d_f16>(npix * 64); NN(ctx, d_a);
        HIPCHK(ctx, hipMemsetAsync(d_a, 0xff, npix * 64 * sizeof(hp3d_f16), ctx->stream));
        CHK(run_conv(ctx, wts, l1, d_img, 3, B, H, W, (float*)d_a, 64, 0, nullptr, nullptr, 1));
        CHK(run_conv(ctx, wts, l2, (const float*)d_a, 64, B, H, W, (float*)d_out, 64, 1, &oh, &ow, 1));
    }
    return finish_op_f16(ctx, d_out, opix, 64, 64, 0, out);
}

int hp3d_maxpool2(hp3d_ctx* ctx, const float* x, int B, int H, int W, int C, float* out) {
    if (!ctx) return HP3D_ERR_ARG;
    if (!x || !out || B < 1 || H < 2 || W < 2 || C < 1) HP3D_FAIL(ctx, HP3D_ERR_ARG, "bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Scratch S(ctx);
    const size_t no = (size_t)B * (H / 2) * (W / 2) * C;
    float* d_x = S.upload(x, (size_t)B * H * W * C); NN(ctx, d_x);
    float* d_o = S.alloc<float>(no); NN(ctx, d_o);
    maxpool2_launch(d_x, B, H, W, C, C, d_o, ctx->stream);
    HIPCHK(ctx, hipMemcpyAsync(out, d_o, no * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    return finish_op(ctx);
}

int hp3d_avgpool8(hp3d_ctx* ctx, const float* x, int B, int H, int W, int C, float* out) {
    if (!ctx) return HP3D_ERR_ARG;
    if (!x || !out || B < 1 || (H % 8) || (W % 8) || C < 1) HP3D_FAIL(ctx, HP3D_ERR_ARG, "bad arguments (H,W %% 8)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Scratch S(ctx);
    const size_t no = (size_t)B * (H / 8) * (W / 8) * C;
    float* d_x = S.upload(x, (size_t)B * H * W * C); NN(ctx, d_x);
    float* d_o = S.alloc<float>(no); NN(ctx, d_o);
    avgpool8_launch(d_x, B, H, W, C, d_o, C, ctx->stream);
    HIPCHK(ctx, hipMemcpyAsync(out, d_o, no * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    return finish_op(ctx);
}

int hp3d_resize_bilinear(hp3d_ctx* ctx, const float* x, int B, int H, int W, int C, int out_h, int out_w, float* out) {
    if (!ctx) return HP3D_ERR_ARG;
    if (!x || !out || B < 1 || H < 1 || W < 1 || C < 1 || out_h < 1 || out_w < 1) HP3D_FAIL(ctx, HP3D_ERR_ARG, "bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Scratch S(ctx);
    const size_t no = (size_t)B * out_h * out_w * C;
    float* d_x = S.upload(x, (size_t)B * H * W * C); NN(ctx, d_x);
    float* d_o = S.alloc<float>(no); NN(ctx, d_o);
    resize_bilinear_launch(d_x, B, H, W, C, C, out_h, out_w, d_o, ctx->stream);
    HIPCHK(ctx, hipMemcpyAsync(out, d_o, no * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    return finish_op(ctx);
}

int hp3d_crop_and_resize(hp3d_ctx* ctx, const float* image, int B, int H, int W, int C, const float* center,
                         const float* scale, int crop_size, float* out) {
    if (!ctx) return HP3D_ERR_ARG;
    if (!image || !center || !scale || !out || B < 1 || H < 2 || W < 2 || C < 1 || crop_size < 1)
        HP3D_FAIL(ctx, HP3D_ERR_ARG, "bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Scratch S(ctx);
    const size_t no = (size_t)B * crop_size * crop_size * C;
    float* d_x = S.upload(image, (size_t)B * H * W * C); NN(ctx, d_x);
    float* d_c = S.upload(center, (size_t)B * 2); NN(ctx, d_c);
    float* d_s = S.upload(scale, (size_t)B); NN(ctx, d_s);
    float* d_o = S.alloc<float>(no); NN(ctx, d_o);
    crop_and_resize_launch(d_x, B, H, W, C, d_c, d_s, crop_size, d_o, ctx->stream);
    HIPCHK(ctx, hipMemcpyAsync(out, d_o, no * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    return finish_op(ctx);
}

int hp3d_mask_from_scoremap(hp3d_ctx* ctx, const float* scoremap, int B, int H, int W, float* mask, float* center,
                            float* crop_size, float* scale, int32_t* seed) {
    if (!ctx) return HP3D_ERR_ARG;
    if (!scoremap || B < 1 || H < 1 || W < 1) HP3D_FAIL(ctx, HP3D_ERR_ARG, "bad arguments");
    if (!(B < H && B < W)) HP3D_FAIL(ctx, HP3D_ERR_ARG, "Scoremap must be [Batch, Width, Height]");  // general.py:210
    if ((long)H * W > (1L << 30)) HP3D_FAIL(ctx, HP3D_ERR_ARG, "map too large (more than 2^30 pixels)");
    const bool global = mask_grow_global(ctx, H, W);
    if (!global && !mask_grow_lds_fits(H, W)) HP3D_FAIL(ctx, HP3D_ERR_ARG, "map too large for the in-LDS mask growth");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Scratch S(ctx);
    const size_t npx = (size_t)B * H * W;
    float* d_sm = S.upload(scoremap, npx * 2); NN(ctx, d_sm);
    MaskBuffers mb;
    mb.argmax_key = S.alloc<unsigned long long>(B); NN(ctx, mb.argmax_key);
    mb.det = S.alloc<unsigned char>(npx); NN(ctx, mb.det);
    mb.fg = nullptr;
    float* d_mask = S.alloc<float>(npx); NN(ctx, d_mask);
    float* d_c = S.alloc<float>((size_t)B * 2); NN(ctx, d_c);
    float* d_cs = S.alloc<float>(B); NN(ctx, d_cs);
    float* d_sc = S.alloc<float>(B); NN(ctx, d_sc);
    int* d_seed = S.alloc<int>((size_t)B * 2); NN(ctx, d_seed);
    seg_softmax_launch(d_sm, B, H, W, mb, ctx->stream);
    if (global) {
        unsigned* d_scr = S.alloc<unsigned>((size_t)B * mask_grow_global_words(H, W)); NN(ctx, d_scr);
        mask_grow_global_launch(mb, B, H, W, ctx->empty_fltmax, d_scr, d_mask, d_c, d_cs, d_sc, d_seed, ctx->stream);
        ++ctx->mask_grow_global_launches;
    } else {
        mask_grow_launch(mb, B, H, W, ctx->empty_fltmax, d_mask, d_c, d_cs, d_sc, d_seed, ctx->stream);
    }
    if (mask) HIPCHK(ctx, hipMemcpyAsync(mask, d_mask, npx * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    if (center) HIPCHK(ctx, hipMemcpyAsync(center, d_c, sizeof(float) * B * 2, hipMemcpyDeviceToHost, ctx->stream));
    if (crop_size) HIPCHK(ctx, hipMemcpyAsync(crop_size, d_cs, sizeof(float) * B, hipMemcpyDeviceToHost, ctx->stream));
    if (scale) HIPCHK(ctx, hipMemcpyAsync(scale, d_sc, sizeof(float) * B, hipMemcpyDeviceToHost, ctx->stream));
    if (seed) HIPCHK(ctx, hipMemcpyAsync(seed, d_seed, sizeof(int) * B * 2, hipMemcpyDeviceToHost, ctx->stream));
    return finish_op(ctx);
}

int hp3d_fc(hp3d_ctx* ctx, const float* x, int B, int Cin, const float* w, const float* bias, int Cout, int act,
            float* out) {
    if (!ctx) return HP3D_ERR_ARG;
    if (!x || !w || !bias || !out || B < 1 || Cin < 1 || Cout < 1) HP3D_FAIL(ctx, HP3D_ERR_ARG, "bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Scratch S(ctx);
    float* d_x = S.upload(x, (size_t)B * Cin); NN(ctx, d_x);
    float* d_w = S.upload(w, (size_t)Cin * Cout); NN(ctx, d_w);
    float* d_b = S.upload(bias, (size_t)Cout); NN(ctx, d_b);
    float* d_o = S.alloc<float>((size_t)B * Cout); NN(ctx, d_o);
    float* d_p = S.alloc<float>(fc_scratch_floats(B, Cin, Cout)); NN(ctx, d_p);
    fc_launch(d_x, B, Cin, Cin, d_w, d_b, Cout, act, d_o, Cout, d_p, ctx->stream);
    HIPCHK(ctx, hipMemcpyAsync(out, d_o, sizeof(float) * (size_t)B * Cout, hipMemcpyDeviceToHost, ctx->stream));
    return finish_op(ctx);
}

int hp3d_argmax2d(hp3d_ctx* ctx, const float* x, int B, int H, int W, int C, int32_t* out_rc) {
    if (!ctx) return HP3D_ERR_ARG;
    if (!x || !out_rc || B < 1 || H < 1 || W < 1 || C < 1) HP3D_FAIL(ctx, HP3D_ERR_ARG, "bad arguments");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Scratch S(ctx);
    float* d_x = S.upload(x, (size_t)B * H * W * C); NN(ctx, d_x);
    int* d_o = S.alloc<int>((size_t)B * C * 2); NN(ctx, d_o);
    argmax2d_launch(d_x, B, H, W, C, C, d_o, ctx->stream);
    HIPCHK(ctx, hipMemcpyAsync(out_rc, d_o, sizeof(int) * (size_t)B * C * 2, hipMemcpyDeviceToHost, ctx->stream));
    return finish_op(ctx);
}

// ---- measurement ---------------------------------------------------------------------------------
int hp3d_set_profiling(hp3d_ctx* ctx, int on) {
    if (!ctx) return HP3D_ERR_ARG;
    if (on != ctx->profiling) prof_reset(ctx);
    ctx->profiling = (on == 2) ? 2 : (on ? 1 : 0);
    return 0;
}
int hp3d_prof_count(hp3d_ctx* ctx) { return ctx ? (int)ctx->prof.size() : 0; }
int hp3d_prof_get(hp3d_ctx* ctx, int i, char* name, int name_cap, char* kernel, int kernel_cap, float* ms,
                  double* flops, double* bytes) {
    if (!ctx || i < 0 || i >= (int)ctx->prof.size()) return HP3D_ERR_ARG;
    const ProfRec& r = ctx->prof[i];
    if (name && name_cap > 0) snprintf(name, name_cap, "%s", r.name.c_str());
    if (kernel && kernel_cap > 0) snprintf(kernel, kernel_cap, "%s", r.kernel.c_str());
    if (ms) {
        HIPCHK(ctx, hipEventSynchronize(r.e1));
        HIPCHK(ctx, hipEventElapsedTime(ms, r.e0, r.e1));
    }
    if (flops) *flops = r.flops;
    if (bytes) *bytes = r.bytes;
    return 0;
}

int hp3d_get_counter(hp3d_ctx* ctx, const char* name, long long* value) {
    if (!ctx || !name || !value) return HP3D_ERR_ARG;
    // {name, counter, + the child context's (every whole-path counter: the second stream's half ran there)}
    static const struct { const char* name; long Counters::*member; bool with_kid; } table[] = {
        {"graph_captures", &Counters::graph_captures, false},
        {"graph_replays", &Counters::graph_replays, false},
        {"lift_overlap_calls", &Counters::lift_overlap_calls, false},
        {"mask_grow_global_launches", &Counters::mask_grow_global_launches, true},
        {"mask_grow_multi_launches", &Counters::mask_grow_multi_launches, false},
        {"conv_h16_launches", &Counters::conv_h16_launches, true},
        {"conv_h16_first_resident_launches", &Counters::conv_h16_first_resident_launches, true},
        {"first_touch_launches", &Counters::first_touch_launches, true},
        {"conv_first_launches", &Counters::conv_first_launches, true},
        {"lift_fused_launches", &Counters::lift_fused_launches, true},
        {"conv_wino4_tail_launches", &Counters::conv_wino4_tail_launches, true},
        {"conv_pw2_launches", &Counters::conv_pw2_launches, true},
        {"conv_wino7_split_launches", &Counters::conv_wino7_split_launches, true},
        {"conv_wino7_launches", &Counters::conv_wino7_launches, true},
        {"fc_tail_launches", &Counters::fc_tail_launches, true},
        {"conv_s2_gemm_launches", &Counters::conv_s2_gemm_launches, true},
        {"conv_wino4s_launches", &Counters::conv_wino4s_launches, true},
        {"conv_wino4s_tail_launches", &Counters::conv_wino4s_tail_launches, true},
        {"conv_wino4_launches", &Counters::conv_wino4_launches, true},
        {"conv_wino2_launches", &Counters::conv_wino2_launches, true},
        {"conv_wino_launches", &Counters::conv_wino_launches, true},
        {"conv_mfma_launches", &Counters::conv_mfma_launches, true},
        {"conv_splitk_reduce_launches", &Counters::conv_splitk_reduce_launches, true},
        {"track_detect_steps", &Counters::track_detect_steps, false},
        {"track_tracked_steps", &Counters::track_tracked_steps, false},
        {"track_hands_detect_steps", &Counters::track_hands_detect_steps, false},
        {"track_hands_tracked_steps", &Counters::track_hands_tracked_steps, false},
        {"crop_u8_launches", &Counters::crop_u8_launches, false},
        {"detect_scale_steps", &Counters::detect_scale_steps, false},
        {"hands_compact_slots_run", &Counters::hands_compact_slots_run, false},
        {"hands_compact_slots_skipped", &Counters::hands_compact_slots_skipped, false},
        {"hands_compact_waits", &Counters::hands_compact_waits, false},
        {"track_partial_frames_run", &Counters::track_partial_frames_run, false},
        {"track_partial_frames_skipped", &Counters::track_partial_frames_skipped, false},
        {"track_hands_partial_frames_run", &Counters::track_hands_partial_frames_run, false},
        {"track_hands_partial_frames_skipped", &Counters::track_hands_partial_frames_skipped, false},
        {"frame_gather_launches", &Counters::frame_gather_launches, false},
        {"crop_nv12_launches", &Counters::crop_nv12_launches, false},
        {"crop_px_launches", &Counters::crop_px_launches, false},
        {"crop_surf_launches", &Counters::crop_surf_launches, false},
    };
    const std::string k(name);
    for (const auto& c : table)
        if (k == c.name) { *value = ctx->*c.member + (c.with_kid && ctx->kid ? ctx->kid->*c.member : 0); return 0; }
#ifdef HP3D_EMU
    if (k == "emu_soff_overreads") { *value = (long)hp3d_emu_soff_overreads; return 0; }     // interpreter only: 16-byte loads that left their buffer through the scalar offset
#endif
    if (k == "comm_ranks") { *value = comm_ranks(ctx); return 0; }
    if (k == "arena_bytes") {          // the frame-sized buffers of this context: the two activation buffers, image, staging, score map, mask, fg, det
        *value = (long long)(4 * (2 * ctx->act_floats + ctx->image_floats + ctx->stage_floats + ctx->large_floats + ctx->mask_floats + ctx->large_floats / 2) + ctx->det_bytes);
        return 0;
    }
    HP3D_FAIL(ctx, HP3D_ERR_ARG, "unknown counter %s", name);
}
int hp3d_get_timing(hp3d_ctx* ctx, float* ms_per_stage, int n) {
    if (!ctx || !ms_per_stage || n < 1) return HP3D_ERR_ARG;
    float acc[HP3D_TIMING_STAGES] = {0.f, 0.f, 0.f, 0.f, 0.f};
    for (const ProfRec& r : ctx->prof) {
        float ms = 0.f;
        HIPCHK(ctx, hipEventSynchronize(r.e1));
        HIPCHK(ctx, hipEventElapsedTime(&ms, r.e0, r.e1));
        int st = 1;                                                        // glue: softmax / mask / crop
        if (r.name.rfind("HandSegNet/", 0) == 0) st = 0;
        else if (r.name.rfind("PoseNet2D/", 0) == 0 || r.name == "kp_upsample") st = 2;
        else if (r.name.rfind("PosePrior", 0) == 0 || r.name.rfind("ViewpointNet/", 0) == 0 || r.name == "lift_epilogue" ||
                 r.name.rfind("fc", 0) == 0) st = 3;
        acc[st] += ms;
        acc[4] += ms;
    }
    for (int i = 0; i < n && i < HP3D_TIMING_STAGES; ++i) ms_per_stage[i] = acc[i];
    return 0;
}

// ---- RCCL (loaded lazily) ----------------------------------------------------------------------------------------
#ifndef HP3D_EMU
namespace {
struct Rccl {
    void* h = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclBroadcast) Broadcast = nullptr;
    decltype(&ncclAllGather) AllGather = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    decltype(&ncclCommCount) CommCount = nullptr;       // optional: the communicator's own idea of its size
};
Rccl* rccl(hp3d_ctx* ctx) {
    static Rccl R;
    if (R.h) return &R;
    // a process that already carries an RCCL (e.g. torch's) gets that one: same SONAME
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    void* h = nullptr;
    for (const char* nm : names)
        if ((h = dlopen(nm, RTLD_NOW | RTLD_GLOBAL))) break;
    if (!h) { set_error(ctx, "librccl not found (dlopen)"); return nullptr; }
    R.GetUniqueId = (decltype(R.GetUniqueId))dlsym(h, "ncclGetUniqueId");
    R.CommInitRank = (decltype(R.CommInitRank))dlsym(h, "ncclCommInitRank");
    R.Broadcast = (decltype(R.Broadcast))dlsym(h, "ncclBroadcast");
    R.AllGather = (decltype(R.AllGather))dlsym(h, "ncclAllGather");
    R.CommDestroy = (decltype(R.CommDestroy))dlsym(h, "ncclCommDestroy");
    R.GetErrorString = (decltype(R.GetErrorString))dlsym(h, "ncclGetErrorString");
    R.CommCount = (decltype(R.CommCount))dlsym(h, "ncclCommCount");
    if (!R.GetUniqueId || !R.CommInitRank || !R.Broadcast || !R.AllGather || !R.CommDestroy || !R.GetErrorString) {
        set_error(ctx, "librccl lacks an expected symbol");
        return nullptr;
    }
    R.h = h;
    return &R;
}
#define NCCLCHK(ctx, R, call)                                                          \
    do {                                                                               \
        ncclResult_t _r = (call);                                                      \
        if (_r != ncclSuccess) HP3D_FAIL(ctx, HP3D_ERR_HIP, "%s: %s", #call, (R)->GetErrorString(_r)); \
    } while (0)
}  // namespace

int hp3d_comm_unique_id(void* id128) {
    if (!id128) return HP3D_ERR_ARG;
    static_assert(sizeof(ncclUniqueId) == HP3D_COMM_ID_BYTES, "ncclUniqueId size");
    Rccl* R = rccl(nullptr);
    if (!R) return HP3D_ERR_UNSUPPORTED;
    ncclUniqueId id;
    if (R->GetUniqueId(&id) != ncclSuccess) { set_error(nullptr, "ncclGetUniqueId failed"); return HP3D_ERR_HIP; }
    memcpy(id128, &id, sizeof(id));
    return 0;
}
int hp3d_comm_init(hp3d_ctx* ctx, int rank, int nranks, const void* id128) {
    if (!ctx || !id128 || nranks < 1 || rank < 0 || rank >= nranks) return HP3D_ERR_ARG;
    if (ctx->comm) HP3D_FAIL(ctx, HP3D_ERR_ARG, "communicator already initialised");
    Rccl* R = rccl(ctx);
    if (!R) return HP3D_ERR_UNSUPPORTED;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ncclUniqueId id;
    memcpy(&id, id128, sizeof(id));
    ncclComm_t c = nullptr;
    NCCLCHK(ctx, R, R->CommInitRank(&c, nranks, id, rank));
    ctx->comm = c; ctx->comm_rank = rank; ctx->comm_size = nranks;
    return 0;
}
int hp3d_bcast_weights(hp3d_ctx* ctx, int root) {
    if (ctx) ++ctx->graph_epoch;
    if (!ctx || !ctx->comm || root < 0 || root >= ctx->comm_size) return HP3D_ERR_ARG;
    Rccl* R = rccl(ctx);
    if (!R) return HP3D_ERR_UNSUPPORTED;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    ncclComm_t c = (ncclComm_t)ctx->comm;
    const bool is_root = ctx->comm_rank == root;
    if (is_root && !ctx->blob) HP3D_FAIL(ctx, HP3D_ERR_WEIGHTS, "root has no finalized weights");
    // header: nets mask (bit 5 = half-precision section live); the blob layout is identical on every rank
    Scratch S(ctx);
    int* d_hdr = S.alloc<int>(2); NN(ctx, d_hdr);
    int hdr[2] = {is_root ? hp3d_nets_mask(ctx) : 0, 0};
    HIPCHK(ctx, hipMemcpyAsync(d_hdr, hdr, sizeof(hdr), hipMemcpyHostToDevice, ctx->stream));
    NCCLCHK(ctx, R, R->Broadcast(d_hdr, d_hdr, 2, ncclInt, root, c, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(hdr, d_hdr, sizeof(hdr), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    const int mask = hdr[0], f16 = (mask & 32) ? 1 : 0;
    if (!ctx->blob) CHK(dev_realloc(ctx, &ctx->blob, ctx->T.blob_floats));
    NCCLCHK(ctx, R, R->Broadcast(ctx->blob, ctx->blob, ctx->T.blob_floats, ncclFloat, root, c, ctx->stream));
    if (f16) {
        if (!ctx->blob16) CHK(dev_realloc(ctx, &ctx->blob16, ctx->T.blob16_halves));
        NCCLCHK(ctx, R, R->Broadcast(ctx->blob16, ctx->blob16, ctx->T.blob16_halves, ncclHalf, root, c, ctx->stream));
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->nets = mask & 31;
    ctx->prec = f16;
    return 0;
}
static int gather_staging(hp3d_ctx* ctx, size_t floats) {
    if (floats > ctx->gather_floats) {
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        CHK(dev_realloc(ctx, &ctx->d_gather, floats));
        ctx->gather_floats = floats;
    }
    return 0;
}
int hp3d_allgather(hp3d_ctx* ctx, const float* send_host, int count, float* recv_host) {
    if (!ctx || !ctx->comm || !send_host || !recv_host || count < 1) return HP3D_ERR_ARG;
    Rccl* R = rccl(ctx);
    if (!R) return HP3D_ERR_UNSUPPORTED;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    CHK(gather_staging(ctx, (size_t)count * (ctx->comm_size + 1)));
    float* d_send = ctx->d_gather;
    float* d_recv = ctx->d_gather + count;
    HIPCHK(ctx, hipMemcpyAsync(d_send, send_host, sizeof(float) * count, hipMemcpyHostToDevice, ctx->stream));
    NCCLCHK(ctx, R, R->AllGather(d_send, d_recv, (size_t)count, ncclFloat, (ncclComm_t)ctx->comm, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(recv_host, d_recv, sizeof(float) * count * ctx->comm_size, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}
int hp3d_allgather_dev(hp3d_ctx* ctx, const float* send_dev, int count, float* recv_host) {
    if (!ctx || !ctx->comm || !send_dev || !recv_host || count < 1) return HP3D_ERR_ARG;
    Rccl* R = rccl(ctx);
    if (!R) return HP3D_ERR_UNSUPPORTED;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    CHK(gather_staging(ctx, (size_t)count * ctx->comm_size));
    float* d_recv = ctx->d_gather;
    NCCLCHK(ctx, R, R->AllGather(send_dev, d_recv, (size_t)count, ncclFloat, (ncclComm_t)ctx->comm, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(recv_host, d_recv, sizeof(float) * count * ctx->comm_size, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}
int hp3d_comm_destroy(hp3d_ctx* ctx) {
    if (!ctx) return HP3D_ERR_ARG;
    if (!ctx->comm) return 0;
    Rccl* R = rccl(ctx);
    if (R) R->CommDestroy((ncclComm_t)ctx->comm);
    ctx->comm = nullptr; ctx->comm_size = 1; ctx->comm_rank = 0;
    return 0;
}
#else   // the CPU interpreter build has no RCCL
int hp3d_comm_unique_id(void*) { return HP3D_ERR_UNSUPPORTED; }
int hp3d_comm_init(hp3d_ctx* ctx, int, int, const void*) { HP3D_FAIL(ctx, HP3D_ERR_UNSUPPORTED, "no RCCL in the CPU interpreter build"); }
int hp3d_bcast_weights(hp3d_ctx* ctx, int) { HP3D_FAIL(ctx, HP3D_ERR_UNSUPPORTED, "no RCCL in the CPU interpreter build"); }
int hp3d_allgather(hp3d_ctx* ctx, const float*, int, float*) { HP3D_FAIL(ctx, HP3D_ERR_UNSUPPORTED, "no RCCL in the CPU interpreter build"); }
int hp3d_allgather_dev(hp3d_ctx* ctx, const float*, int, float*) { HP3D_FAIL(ctx, HP3D_ERR_UNSUPPORTED, "no RCCL in the CPU interpreter build"); }
int hp3d_comm_destroy(hp3d_ctx*) { return 0; }
#endif

uint32_t hp3d_crc32c(const void* data, size_t n) {
    static uint32_t T[8][256];
    static bool init = false;
    if (!init) {
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ 0x82F63B78u : c >> 1;
            T[0][i] = c;
        }
        for (uint32_t i = 0; i < 256; ++i)
            for (int t = 1; t < 8; ++t) T[t][i] = (T[t - 1][i] >> 8) ^ T[0][T[t - 1][i] & 0xFF];
        init = true;
    }
    const unsigned char* p = (const unsigned char*)data;
    uint32_t crc = 0xFFFFFFFFu;
    while (n >= 8) {                       // slicing-by-8
        uint32_t lo, hi;
        memcpy(&lo, p, 4); memcpy(&hi, p + 4, 4);
        lo ^= crc;
        crc = T[7][lo & 0xFF] ^ T[6][(lo >> 8) & 0xFF] ^ T[5][(lo >> 16) & 0xFF] ^ T[4][lo >> 24] ^
              T[3][hi & 0xFF] ^ T[2][(hi >> 8) & 0xFF] ^ T[1][(hi >> 16) & 0xFF] ^ T[0][hi >> 24];
        p += 8; n -= 8;
    }
    while (n--) crc = T[0][(crc ^ *p++) & 0xFF] ^ (crc >> 8);
    return crc ^ 0xFFFFFFFFu;
}

}  // extern "C"

static long long comm_ranks(hp3d_ctx* ctx) {
#ifndef HP3D_EMU
    if (!ctx || !ctx->comm) return 0;
    Rccl* R = rccl(ctx);
    int n = 0;
    if (R && R->CommCount && R->CommCount((ncclComm_t)ctx->comm, &n) == ncclSuccess) return n;
    return ctx->comm_size;
#else
    (void)ctx;
    return 0;
#endif
}
