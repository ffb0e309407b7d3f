// glue.hip -- the HBM-bound / latency-bound stages between the MFMA convolutions.
// Everything here is compiled with -ffp-contract=off: the reference evaluates these
// expressions op by op in float32 (TF 1.3 CPU/GPU kernels), and the box / interpolation
// arithmetic feeds discontinuous decisions (row validity, floor/ceil), so no FMA contraction.
#include "hp3d_common.h"
#include <cstring>
#include <type_traits>

namespace {

__device__ __forceinline__ float leaky(float x) { return fmaxf(x, HP3D_LEAKY_SLOPE * x); }

// ---------------------------------------------------------------------------------------
// conv_naive: one thread per output element; HWIO weights as given by the caller.
// Debug cross-check for conv_mfma (hp3d_set_option conv_impl=naive) -- never a fallback.
HP3D_KERNEL(256)
void conv_naive_kernel(const float* x, int B, int H, int W, int Cin, int in_cs, const float* w, const float* bias,
                       int k, int stride, int Cout, int act, float* out, int out_cs, int Ho, int Wo,
                       int pad_t, int pad_l) {
    const long total = (long)B * Ho * Wo * Cout;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int co = (int)(i % Cout);
        long r = i / Cout;
        const int ox = (int)(r % Wo); r /= Wo;
        const int oy = (int)(r % Ho);
        const int b = (int)(r / Ho);
        float acc = 0.f;
        for (int ky = 0; ky < k; ++ky) {
            const int iy = oy * stride - pad_t + ky;
            if (iy < 0 || iy >= H) continue;
            for (int kx = 0; kx < k; ++kx) {
                const int ix = ox * stride - pad_l + kx;
                if (ix < 0 || ix >= W) continue;
                const float* xp = x + (((size_t)b * H + iy) * W + ix) * in_cs;
                const float* wp = w + ((size_t)(ky * k + kx) * Cin) * Cout + co;
                for (int c = 0; c < Cin; ++c) acc = fmaf(xp[c], wp[(size_t)c * Cout], acc);
            }
        }
        acc += bias[co];
        if (act) acc = leaky(acc);
        out[(((size_t)b * Ho + oy) * Wo + ox) * out_cs + co] = acc;
    }
}

// split-K epilogue of conv_mfma / the Winograd kernels: fixed-order sum over the K slices, then bias + leaky-ReLU.
// VEC = 4: a thread owns four consecutive couts (16-byte loads / stores; Cout, out_cs, cout_store multiples of 4, aligned pointers).
// Up to eight slices are requested before the first addition (same order of additions): one load per addition is a chain of
// `ksplit` dependent memory round trips -- 10 us for a 16-way split of a few hundred KB, which is what 25 of PoseNet2D's 56 launches
// at B = 1 were (round 5).
template <int VEC>
HP3D_KERNEL(256)
void conv_splitk_reduce_kernel(const float* partial, int ksplit, long npix, int Cout, const float* bias, int act,
                               float* out, int out_cs, int cout_store) {
    typedef typename std::conditional<VEC == 4, f32x4, float>::type vec_t;
    const int cvec = cout_store / VEC;
    const long total = npix * cvec;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int co = (int)(i % cvec) * VEC;
        const long pix = i / cvec;
        const float* src = partial + (size_t)pix * Cout + co;
        const size_t zs = (size_t)npix * Cout;
        vec_t v = {};
        int z = 0;
        for (; z + 8 <= ksplit; z += 8) {
            vec_t t[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) t[u] = *(const vec_t*)(src + (size_t)(z + u) * zs);
#pragma unroll
            for (int u = 0; u < 8; ++u) v += t[u];
        }
        if (z + 4 <= ksplit) {
            vec_t t[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) t[u] = *(const vec_t*)(src + (size_t)(z + u) * zs);
#pragma unroll
            for (int u = 0; u < 4; ++u) v += t[u];
            z += 4;
        }
        for (; z < ksplit; ++z) v += *(const vec_t*)(src + (size_t)z * zs);
        v += *(const vec_t*)(bias + co);
        if (act) {
            if constexpr (VEC == 4) { for (int j = 0; j < 4; ++j) v[j] = leaky(v[j]); }
            else v = leaky(v);
        }
        *(vec_t*)(out + pix * out_cs + co) = v;
    }
}

// the same followed by the 2x2 / 2 max-pool of the layer (NetworkOps.max_pool, utils/general.py:61-65): partial sums are
// [ksplit][B, H, W][Cout] at conv resolution, the output is [B, H/2, W/2] -- each of the four pixels is summed in split order,
// biased and activated exactly like the unpooled form, then the maximum is taken
HP3D_KERNEL(256)
void conv_splitk_reduce_pool_kernel(const float* partial, int ksplit, int B, int H, int W, int Cout, const float* bias, int act,
                                    float* out, int out_cs, int cout_store) {
    const int Hp = H / 2, Wp = W / 2;
    const long npix = (long)B * H * W, total = (long)B * Hp * Wp * cout_store;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int co = (int)(i % cout_store);
        long r = i / cout_store;
        const int ox = (int)(r % Wp); r /= Wp;
        const int oy = (int)(r % Hp);
        const int b = (int)(r / Hp);
        float m = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const long pix = ((long)b * H + 2 * oy + (q >> 1)) * W + 2 * ox + (q & 1);
            float v = 0.f;
            for (int z = 0; z < ksplit; ++z) v += partial[((size_t)z * npix + pix) * Cout + co];
            v += bias[co];
            if (act) v = leaky(v);
            m = q == 0 ? v : fmaxf(m, v);
        }
        out[(((long)b * Hp + oy) * Wp + ox) * out_cs + co] = m;
    }
}

// ---------------------------------------------------------------------------------------
// 2x2/2 VALID max-pool (utils/general.py:61-65), standalone (the pipeline uses the fused epilogue)
HP3D_KERNEL(256)
void maxpool2_kernel(const float* x, int B, int H, int W, int C, int in_cs, float* out) {
    const int Ho = H / 2, Wo = W / 2;
    const long total = (long)B * Ho * Wo * C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        long r = i / C;
        const int ox = (int)(r % Wo); r /= Wo;
        const int oy = (int)(r % Ho);
        const int b = (int)(r / Ho);
        const float* p = x + (((size_t)b * H + 2 * oy) * W + 2 * ox) * in_cs + c;
        const float m0 = fmaxf(p[0], p[in_cs]);
        const float m1 = fmaxf(p[(size_t)W * in_cs], p[(size_t)W * in_cs + in_cs]);
        out[i] = fmaxf(m0, m1);
    }
}

// 8x8/8 average pool on sizes divisible by 8 (nets/PosePriorNetwork.py:61); row-major f32 sum
HP3D_KERNEL(256)
void avgpool8_kernel(const float* x, int B, int H, int W, int C, float* out, int out_cs) {
    const int Ho = H / 8, Wo = W / 8;
    const long total = (long)B * Ho * Wo * C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        long r = i / C;
        const int ox = (int)(r % Wo); r /= Wo;
        const int oy = (int)(r % Ho);
        const int b = (int)(r / Ho);
        float s = 0.f;
        for (int dy = 0; dy < 8; ++dy)
            for (int dx = 0; dx < 8; ++dx)
                s += x[(((size_t)b * H + oy * 8 + dy) * W + ox * 8 + dx) * C + c];
        out[(((size_t)b * Ho + oy) * Wo + ox) * out_cs + c] = s / 64.f;
    }
}

// TF 1.3 ResizeBilinear, align_corners=False
__device__ __forceinline__ void resize_coord(int o, float scale, int in_n, int& lo, int& hi, float& t) {
    const float src = (float)o * scale;
    lo = (int)floorf(src);
    hi = min(lo + 1, in_n - 1);
    t = src - (float)lo;
}

template <typename IDX>      // IDX = unsigned when the element count fits 32 bits (3x fewer index instructions)
HP3D_KERNEL(256)
void resize_bilinear_kernel(const float* x, int B, int H, int W, int C, int in_cs, int oh, int ow, float* out) {
    const float hscale = (float)H / (float)oh, wscale = (float)W / (float)ow;
    const IDX total = (IDX)B * oh * ow * C;
    for (IDX i = (IDX)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (IDX)gridDim.x * blockDim.x) {
        const int c = (int)(i % (IDX)C);
        IDX r = i / (IDX)C;
        const int ox = (int)(r % (IDX)ow); r /= (IDX)ow;
        const int oy = (int)(r % (IDX)oh);
        const int b = (int)(r / (IDX)oh);
        int y0, y1, x0, x1; float ty, tx;
        resize_coord(oy, hscale, H, y0, y1, ty);
        resize_coord(ox, wscale, W, x0, x1, tx);
        const float* xb = x + (size_t)b * H * W * in_cs + c;
        const float tl = xb[((size_t)y0 * W + x0) * in_cs], tr = xb[((size_t)y0 * W + x1) * in_cs];
        const float bl = xb[((size_t)y1 * W + x0) * in_cs], br = xb[((size_t)y1 * W + x1) * in_cs];
        const float top = tl + (tr - tl) * tx;
        const float bot = bl + (br - bl) * tx;
        out[i] = top + (bot - top) * ty;
    }
}

// The same arithmetic, one workgroup per output ROW: its two source rows (2 x W x C floats) and the 3 x ow column terms sit in LDS, every
// thread makes four consecutive values of the row's ow x C floats and stores them as 16 bytes.  For the 8x up-sampling of the key-point
// score maps (32 x 32 x 21 -> 256 x 256 x 21, 176 MB per 32 images: the element kernel above spends its time on three integer divisions
// and four gathered global loads per value, 1.6 TB/s) this is a streaming store.  Needs (ow x C) % 4 == 0 and 2 W C + 3 ow floats of LDS.
HP3D_KERNEL(256)
void resize_bilinear_rows_kernel(const float* x, int H, int W, int C, int in_cs, int oh, int ow, float* out, float inv_c) {
    HP3D_DYN_SMEM(sm);
    float* rows = sm;                             // [2][W][C]
    int* cx0 = (int*)(sm + 2 * W * C);            // [ow] x0 * C, [ow] x1 * C
    int* cx1 = cx0 + ow;
    float* ctx = (float*)(cx1 + ow);              // [ow] tx
    const int oy = blockIdx.x, b = blockIdx.y;
    const float hscale = (float)H / (float)oh, wscale = (float)W / (float)ow;
    int y0, y1; float ty;
    resize_coord(oy, hscale, H, y0, y1, ty);
    const float* xb = x + (size_t)b * H * W * in_cs;
    for (int i = threadIdx.x; i < W * C; i += blockDim.x) {
        const int px = (int)(((float)i + 0.5f) * inv_c), c = i - px * C;
        rows[i] = xb[((size_t)y0 * W + px) * in_cs + c];
        rows[W * C + i] = xb[((size_t)y1 * W + px) * in_cs + c];
    }
    for (int ox = threadIdx.x; ox < ow; ox += blockDim.x) {
        int x0, x1; float tx;
        resize_coord(ox, wscale, W, x0, x1, tx);
        cx0[ox] = x0 * C; cx1[ox] = x1 * C; ctx[ox] = tx;
    }
    __syncthreads();
    float* orow = out + ((size_t)b * oh + oy) * (size_t)ow * C;
    const float* r0 = rows;
    const float* r1 = rows + W * C;
    for (int q4 = threadIdx.x * 4; q4 < ow * C; q4 += blockDim.x * 4) {
        int ox = (int)(((float)q4 + 0.5f) * inv_c), c = q4 - ox * C;
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int a0 = cx0[ox] + c, a1 = cx1[ox] + c;
            const float tx = ctx[ox];
            const float tl = r0[a0], tr = r0[a1], bl = r1[a0], br = r1[a1];
            const float top = tl + (tr - tl) * tx;
            const float bot = bl + (br - bl) * tx;
            v[e] = top + (bot - top) * ty;
            if (++c == C) { c = 0; ++ox; }
        }
        *(f32x4*)(orow + q4) = v;
    }
}

// Input pre-processing on device: uint8 image -> `x/255 - 0.5` (data/BinaryDbReader.py:182,
// run.py:59) -> tf.image.resize_images to the network size (eval_full.py:50, eval2d.py:53), fused:
// 4x less H2D traffic, no float image round trip.  Same float32 op order as the oracle (bit-exact).
HP3D_KERNEL(256)
void preprocess_u8_kernel(const unsigned char* img, int B, int H, int W, int oh, int ow, float* out) {
    const float hscale = (float)H / (float)oh, wscale = (float)W / (float)ow;
    const long total = (long)B * oh * ow * 3;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % 3);
        long r = i / 3;
        const int ox = (int)(r % ow); r /= ow;
        const int oy = (int)(r % oh);
        const int b = (int)(r / oh);
        int y0, y1, x0, x1; float ty, tx;
        resize_coord(oy, hscale, H, y0, y1, ty);
        resize_coord(ox, wscale, W, x0, x1, tx);
        const unsigned char* ib = img + (size_t)b * H * W * 3 + c;
        const float tl = (float)ib[((size_t)y0 * W + x0) * 3] / 255.0f - 0.5f, tr = (float)ib[((size_t)y0 * W + x1) * 3] / 255.0f - 0.5f;
        const float bl = (float)ib[((size_t)y1 * W + x0) * 3] / 255.0f - 0.5f, br = (float)ib[((size_t)y1 * W + x1) * 3] / 255.0f - 0.5f;
        const float top = tl + (tr - tl) * tx;
        const float bot = bl + (br - bl) * tx;
        out[i] = (oh == H && ow == W) ? tl : top + (bot - top) * ty;
    }
}

// ---- NV12 frames ------------------------------------------------------------------------------------------------------
// Pixel (r, c) of frame `fr` of an NV12 surface as three uint8 channels -- the one place the colour rule of include/hp3d.h is written:
// Y = y[r pitch + c]; U, V = the byte pair at uv[(r >> 1) pitch + (c & ~1)] (one 2-byte load: chroma is replicated over its 2 x 2 block,
// never interpolated); C = Y - yoff, D = U - 128, E = V - 128; channel = clamp((ky C + cu D + cv E + 128) >> 8, 0, 255), int32, the
// shift arithmetic.  Only bytes [0, W) of a row are read (W even: c | 1 < W).
struct Rgb8 { int r, g, b; };
__device__ __forceinline__ int nv12_clamp8(int v) { return min(max(v >> 8, 0), 255); }
__device__ __forceinline__ Rgb8 nv12_convert(const Nv12Src& P, int Y, int U, int V) {
    const int C = P.ky * (Y - P.yoff) + 128, D = U - 128, E = V - 128;
    Rgb8 o;
    o.r = nv12_clamp8(C + P.rv * E);
    o.g = nv12_clamp8(C + P.gu * D + P.gv * E);
    o.b = nv12_clamp8(C + P.bu * D);
    return o;
}
__device__ __forceinline__ Rgb8 nv12_pixel(const Nv12Src& P, size_t fr, int r, int c) {
    const size_t fb = fr * P.frame_stride;
    const int Y = P.y[fb + (size_t)r * P.pitch + c];
    unsigned char uv[2];
    __builtin_memcpy(uv, P.uv + fb + (size_t)(r >> 1) * P.pitch + (c & ~1), 2);
    return nv12_convert(P, Y, uv[0], uv[1]);
}
// a uint8 channel as a network value, as preprocess_u8_kernel makes it
__device__ __forceinline__ float u8_norm(int ch) { return (float)ch / 255.0f - 0.5f; }

// crop_image_from_xy -> tf.image.crop_and_resize (utils/general.py:163-196, App. B.4).  One body for both pixel types: `tap(pixel, c)` is
// the value of channel c of pixel `pixel` of the whole batch -- a float32 image as it is, a uint8 frame normalised as
// preprocess_u8_kernel does at equal sizes (x / 255 - 0.5, float32 op by op), so that the crop straight from a uint8 frame equals
// preprocess_u8 -> crop_and_resize bit for bit without the normalised float frame ever existing (25 MB at 1080x1920).  The
// extrapolation value 0 is a normalised value.
struct TapF32 {
    const float* img; int C;
    static constexpr bool PIXEL = false;
    __device__ __forceinline__ float operator()(size_t pixel, int c) const { return img[pixel * C + c]; }
};
struct TapU8 {
    const unsigned char* img; int C;
    static constexpr bool PIXEL = false;
    __device__ __forceinline__ float operator()(size_t pixel, int c) const { return (float)img[pixel * C + c] / 255.0f - 0.5f; }
};
// An NV12 tap hands back a whole pixel: its three channels come from one conversion (four conversions per output pixel, not twelve),
// each normalised as TapU8 does -- the crop equals crop_and_resize_u8 on the converted frame bit for bit.
struct TapNv12 {
    Nv12Src P;
    static constexpr bool PIXEL = true;
    __device__ __forceinline__ void pixel(size_t fr, int r, int c, float* v) const {
        const Rgb8 p = nv12_pixel(P, fr, r, c);
        v[0] = u8_norm(p.r); v[1] = u8_norm(p.g); v[2] = u8_norm(p.b);
    }
};
// ---- packed 8-bit frames ----------------------------------------------------------------------------------------------
// Pixel (r, c) of frame `fr` of a packed surface as three uint8 channels.  wide (4-byte pixels on a 4-byte grid): ONE 32-bit load, the
// channels by shifts (byte k of a little-endian word is bits 8 k ...); otherwise three byte loads, so that a 3-byte pixel never reaches
// past its row.  The fourth byte of a 4-byte pixel is never looked at.
__device__ __forceinline__ Rgb8 px_unpack(const PxSrc& P, unsigned w) {
    Rgb8 o;
    o.r = (int)((w >> (8 * P.ro)) & 255u); o.g = (int)((w >> (8 * P.go)) & 255u); o.b = (int)((w >> (8 * P.bo)) & 255u);
    return o;
}
__device__ __forceinline__ Rgb8 px_pixel(const PxSrc& P, size_t fr, int r, int c) {
    const unsigned char* p = P.px + fr * P.frame_stride + (size_t)r * P.pitch + (size_t)c * P.pixel_bytes;
    if (P.wide) {
        unsigned w;
        __builtin_memcpy(&w, __builtin_assume_aligned(p, 4), 4);
        return px_unpack(P, w);
    }
    Rgb8 o;
    o.r = p[P.ro]; o.g = p[P.go]; o.b = p[P.bo];
    return o;
}
// A packed tap hands back a whole pixel, as TapNv12 does: one fetch per tap, each channel normalised as TapU8 does -- the crop equals
// crop_and_resize_u8 on the repacked frame bit for bit.
struct TapPx {
    PxSrc P;
    static constexpr bool PIXEL = true;
    __device__ __forceinline__ void pixel(size_t fr, int r, int c, float* v) const {
        const Rgb8 p = px_pixel(P, fr, r, c);
        v[0] = u8_norm(p.r); v[1] = u8_norm(p.g); v[2] = u8_norm(p.b);
    }
};
// ---- a batch of separate surfaces, formats mixed -------------------------------------------------------------------------
// Frame `fr` is record S.rec[fr]: a packed surface or an NV12 one, at its own address and pitch.  The record is seen through a one-frame
// PxSrc / Nv12Src view (frame stride 0, frame 0), so the unpack and the colour rule stay written once, in px_pixel and nv12_pixel.
__device__ __forceinline__ PxSrc surf_px(const SurfRec& R) { return PxSrc{R.data, R.pitch, 0, R.pixel_bytes, R.ro, R.go, R.bo, R.wide}; }
__device__ __forceinline__ Nv12Src surf_nv12(const SurfSrc& S, const SurfRec& R) {
    return Nv12Src{R.data, R.chroma, R.pitch, 0, S.ky, S.yoff, S.rv, S.gu, S.gv, S.bu};
}
__device__ __forceinline__ Rgb8 surf_pixel(const SurfSrc& S, const SurfRec& R, int r, int c) {
    return R.nv12 ? nv12_pixel(surf_nv12(S, R), 0, r, c) : px_pixel(surf_px(R), 0, r, c);
}
// A surface tap: frame(fr) reads the record ONCE per output pixel into registers; its four taps then cost one fetch each, as TapPx's and
// TapNv12's do -- no second dependent load per tap.  A 256 x 256 crop is a whole number of workgroups, so the record and the format
// branch are uniform over a workgroup of the tracking steps' crops.
struct TapSurfFrame {
    SurfSrc S;
    SurfRec R;
    __device__ __forceinline__ void pixel(size_t, int r, int c, float* v) const {
        const Rgb8 p = surf_pixel(S, R, r, c);
        v[0] = u8_norm(p.r); v[1] = u8_norm(p.g); v[2] = u8_norm(p.b);
    }
};
struct TapSurf {
    SurfSrc S;
    static constexpr bool PIXEL = true;
    __device__ __forceinline__ TapSurfFrame frame(size_t fr) const { return TapSurfFrame{S, S.rec[fr]}; }
    __device__ __forceinline__ void pixel(size_t fr, int r, int c, float* v) const { frame(fr).pixel(0, r, c, v); }
};
// what the four taps of one output pixel are read through: the tap itself, or a surface tap bound to its frame's record
template <class Tap>
__device__ __forceinline__ const Tap& tap_frame(const Tap& tap, size_t) { return tap; }
__device__ __forceinline__ TapSurfFrame tap_frame(const TapSurf& tap, size_t fr) { return tap.frame(fr); }
// the four taps of an output pixel of a PIXEL tap, interpolated as crop_and_resize_body does per channel
template <class Tap>
__device__ __forceinline__ void crop_pixel_taps(const Tap& tap0, size_t fr, int ty0, int ty1, int tx0, int tx1, float ly, float lx, float* o) {
    const auto& tap = tap_frame(tap0, fr);
    float tl[3], tr[3], bl[3], br[3];
    tap.pixel(fr, ty0, tx0, tl); tap.pixel(fr, ty0, tx1, tr);
    tap.pixel(fr, ty1, tx0, bl); tap.pixel(fr, ty1, tx1, br);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float top = tl[c] + (tr[c] - tl[c]) * lx;
        const float bot = bl[c] + (br[c] - bl[c]) * lx;
        o[c] = top + (bot - top) * ly;
    }
}
template <class Tap>
__device__ __forceinline__ void crop_and_resize_body(const Tap tap, int B, int H, int W, int C, const float* center, const float* scale,
                                                     int crop, float* out, int boxes_per_image) {
    const long total = (long)B * crop * crop;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int x = (int)(i % crop);
        long r = i / crop;
        const int y = (int)(r % crop);
        const int b = (int)(r / crop);
        // box arithmetic, float32 op by op (utils/general.py:182-190)
        const float cs = (float)crop / scale[b];
        const float half = floorf(cs / 2.0f);
        float y1 = center[b * 2 + 0] - half, y2 = y1 + cs;
        float x1 = center[b * 2 + 1] - half, x2 = x1 + cs;
        y1 = y1 / (float)H; y2 = y2 / (float)H; x1 = x1 / (float)W; x2 = x2 / (float)W;
        const float hs = (crop > 1) ? (y2 - y1) * (float)(H - 1) / (float)(crop - 1) : 0.f;
        const float ws = (crop > 1) ? (x2 - x1) * (float)(W - 1) / (float)(crop - 1) : 0.f;
        const float in_y = (crop > 1) ? y1 * (float)(H - 1) + (float)y * hs : 0.5f * (y1 + y2) * (float)(H - 1);
        const float in_x = (crop > 1) ? x1 * (float)(W - 1) + (float)x * ws : 0.5f * (x1 + x2) * (float)(W - 1);
        float* o = out + (size_t)i * C;
        const bool ok = in_y >= 0.f && in_y <= (float)(H - 1) && in_x >= 0.f && in_x <= (float)(W - 1);
        if (!ok) {
            for (int c = 0; c < C; ++c) o[c] = 0.f;
            continue;
        }
        const int ty0 = (int)floorf(in_y), ty1 = (int)ceilf(in_y);
        const int tx0 = (int)floorf(in_x), tx1 = (int)ceilf(in_x);
        const float ly = in_y - (float)ty0, lx = in_x - (float)tx0;
        // box b crops image b / boxes_per_image (the K hands of a frame come from the one frame)
        if constexpr (Tap::PIXEL) {
            crop_pixel_taps(tap, (size_t)(boxes_per_image == 1 ? b : b / boxes_per_image), ty0, ty1, tx0, tx1, ly, lx, o);
        } else {
            const size_t ib = (size_t)(boxes_per_image == 1 ? b : b / boxes_per_image) * H * W;
            for (int c = 0; c < C; ++c) {
                const float tl = tap(ib + (size_t)ty0 * W + tx0, c), tr = tap(ib + (size_t)ty0 * W + tx1, c);
                const float bl = tap(ib + (size_t)ty1 * W + tx0, c), br = tap(ib + (size_t)ty1 * W + tx1, c);
                const float top = tl + (tr - tl) * lx;
                const float bot = bl + (br - bl) * lx;
                o[c] = top + (bot - top) * ly;
            }
        }
    }
}
HP3D_KERNEL(256)
void crop_and_resize_kernel(const float* img, int B, int H, int W, int C, const float* center, const float* scale,
                            int crop, float* out, int boxes_per_image) {
    crop_and_resize_body(TapF32{img, C}, B, H, W, C, center, scale, crop, out, boxes_per_image);
}
HP3D_KERNEL(256)
void crop_and_resize_u8_kernel(const unsigned char* img, int B, int H, int W, const float* center, const float* scale,
                               int crop, float* out, int boxes_per_image) {
    crop_and_resize_body(TapU8{img, 3}, B, H, W, 3, center, scale, crop, out, boxes_per_image);
}
HP3D_KERNEL(256)
void crop_and_resize_nv12_kernel(const Nv12Src src, int B, int H, int W, const float* center, const float* scale, int crop, float* out,
                                 int boxes_per_image) {
    crop_and_resize_body(TapNv12{src}, B, H, W, 3, center, scale, crop, out, boxes_per_image);
}
HP3D_KERNEL(256)
void crop_and_resize_px_kernel(const PxSrc src, int B, int H, int W, const float* center, const float* scale, int crop, float* out,
                               int boxes_per_image) {
    crop_and_resize_body(TapPx{src}, B, H, W, 3, center, scale, crop, out, boxes_per_image);
}
HP3D_KERNEL(256)
void crop_and_resize_surf_kernel(const SurfSrc src, int B, int H, int W, const float* center, const float* scale, int crop, float* out,
                                 int boxes_per_image) {
    crop_and_resize_body(TapSurf{src}, B, H, W, 3, center, scale, crop, out, boxes_per_image);
}

HP3D_KERNEL(256)
void copy_channels_kernel(const float* in, long npix, int C, int in_cs, float* out, int out_cs) {
    const long total = npix * C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const long p = i / C;
        out[p * out_cs + c] = in[p * in_cs + c];
    }
}

// float32 [npix, in_cs] channels 0..C-1 -> half [npix, out_cs] (score map fed back into the f16 concat buffer)
HP3D_KERNEL(256)
void cvt_channels_f16_kernel(const float* in, long npix, int C, int in_cs, hp3d_f16* out, int out_cs) {
    const long total = npix * C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C);
        const long p = i / C;
        out[p * out_cs + c] = (hp3d_f16)in[p * in_cs + c];
    }
}

// [npix, C] -> [npix, out_cs] zero padded
HP3D_KERNEL(256)
void pad_channels_kernel(const float* in, long npix, int C, float* out, int out_cs) {
    const long total = npix * out_cs;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int c = (int)(i % out_cs);
        const long p = i / out_cs;
        out[i] = (c < C) ? in[p * C + c] : 0.f;
    }
}

// ---------------------------------------------------------------------------------------
// Segmentation post-processing (utils/general.py:233-245): 2-class softmax in float32 with a
// correctly rounded exp (oracle/tf_ops.py:exp_f32_cr), detmap = round-half-even(fg), and the
// first arg-max of fg over the row-major flattened map as a 64-bit key
//    key = fg_bits << 32 | (0xFFFFFFFF - flat_index)       (fg >= 0 so its bits order like uints)
__device__ __forceinline__ float exp_cr(float x) { return (float)exp((double)x); }

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long k) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = __shfl_xor(k, off);
        k = (o > k) ? o : k;
    }
    return k;
}

// One atomicMax per WORKGROUP on the image's key (round 5: one per wave -- 256 serialised 64-bit atomics per image and address -- was two
// thirds of seg_upsample_softmax's 0.07 ms: without them the kernel takes 0.025, timing ablations `scripts/micro/r05_variants/seg_abl.sh`).
// The maximum does not depend on the order: deterministic as before.  Every thread of the workgroup must call it.
__device__ __forceinline__ void block_max_key(unsigned long long* key, unsigned long long best) {
    __shared__ unsigned long long s_best[16];
    best = wave_max_u64(best);
    const int wave = threadIdx.x >> 6, nwave = (blockDim.x + 63) >> 6;
    if ((threadIdx.x & 63) == 0) s_best[wave] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < nwave; ++i) best = s_best[i] > best ? s_best[i] : best;
        atomicMax(key, best);
    }
}

__device__ __forceinline__ void softmax_det_key(float l0, float l1, unsigned idx, float& fg, unsigned char& det,
                                                unsigned long long& key) {
    const float m = fmaxf(l0, l1);
    const float e0 = exp_cr(l0 - m), e1 = exp_cr(l1 - m);
    const float s = e0 + e1;
    fg = e1 / s;
    det = (unsigned char)(rintf(fg) == 1.0f);
    key = ((unsigned long long)__float_as_uint(fg) << 32) | (unsigned long long)(0xFFFFFFFFu - idx);
}

// small [B,hs,ws,cs] (channels 0,1) --x8 legacy bilinear--> hand_scoremap [B,H,W,2] (+ det, key)
HP3D_KERNEL(256)
void seg_upsample_softmax_kernel(const float* small, int B, int hs, int ws, int cs, int H, int W,
                                 float* large, unsigned char* det, float* fgout, unsigned long long* keys) {
    const int b = blockIdx.y;
    const float hscale = (float)hs / (float)H, wscale = (float)ws / (float)W;
    const int npx = H * W;
    unsigned long long best = 0ull;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < npx; i += gridDim.x * blockDim.x) {
        const int oy = i / W, ox = i - oy * W;
        int y0, y1, x0, x1; float ty, tx;
        resize_coord(oy, hscale, hs, y0, y1, ty);
        resize_coord(ox, wscale, ws, x0, x1, tx);
        const float* sb = small + (size_t)b * hs * ws * cs;
        float l[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const float tl = sb[((size_t)y0 * ws + x0) * cs + c], tr = sb[((size_t)y0 * ws + x1) * cs + c];
            const float bl = sb[((size_t)y1 * ws + x0) * cs + c], br = sb[((size_t)y1 * ws + x1) * cs + c];
            const float top = tl + (tr - tl) * tx;
            const float bot = bl + (br - bl) * tx;
            l[c] = top + (bot - top) * ty;
        }
        const size_t o = (size_t)b * npx + i;
        if (large) { large[o * 2] = l[0]; large[o * 2 + 1] = l[1]; }
        float fg; unsigned char d; unsigned long long key;
        softmax_det_key(l[0], l[1], (unsigned)i, fg, d, key);
        det[o] = d;
        if (fgout) fgout[o] = fg;
        best = key > best ? key : best;
    }
    block_max_key(&keys[b], best);
}

HP3D_KERNEL(256)
void seg_softmax_kernel(const float* large, int B, int H, int W, unsigned char* det, float* fgout,
                        unsigned long long* keys) {
    const int b = blockIdx.y;
    const int npx = H * W;
    unsigned long long best = 0ull;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < npx; i += gridDim.x * blockDim.x) {
        const size_t o = (size_t)b * npx + i;
        float fg; unsigned char d; unsigned long long key;
        softmax_det_key(large[o * 2], large[o * 2 + 1], (unsigned)i, fg, d, key);
        det[o] = d;
        if (fgout) fgout[o] = fg;
        best = key > best ? key : best;
    }
    block_max_key(&keys[b], best);
}

// ---------------------------------------------------------------------------------------
// Seeded geodesic growth + bounding box (utils/general.py:247-328), one workgroup per image.
// O_0 = {seed};  O_{j+1} = det AND dilate21x21(O_j), j < max(H,W)//10 passes, bit-packed in LDS;
// stops early at a fix-point (exactly equivalent: the iteration is deterministic).
// Row r of the bitmap is WW = ceil(W/32) words + ONE zero guard word (pitch P = WW + 1): pixel x is bit x%32 of word x/32; the guard word is
// the right neighbour of the row's last word and the left neighbour of the next row's first, so the horizontal pass reads its neighbours
// without knowing its column (round 5: `w % WW` and `u / WW` per word and pass were a third of the pass's instructions).
// The end of both mask-growth kernels: the [H,W] float mask (optional) from the bitmap `obj` (row pitch P words), and
// calc_center_bb + scale_from_crop_size (nets/ColorHandPose3DNetwork.py:82-85) from the mask's bounding box (rmax < 0: empty mask).
// Every thread of the workgroup calls it after the box is final.
__device__ __forceinline__ void mask_grow_epilogue(const unsigned* obj, int P, int b, int H, int W, int rmin, int rmax, int cmin, int cmax,
                                                   int sy, int sx, int empty_fltmax, float* mask_out, float* center, float* crop_size,
                                                   float* scale, int* seed_out) {
    const int tid = threadIdx.x, nthr = blockDim.x;
    if (mask_out) {
        float* mo = mask_out + (size_t)b * H * W;
        for (int i = tid; i < H * W; i += nthr) {
            const int y = i / W, x = i - y * W;
            mo[i] = (obj[y * P + (x >> 5)] >> (x & 31)) & 1u ? 1.f : 0.f;
        }
    }
    if (tid == 0) {
        float cx, cy, sz;
        if (rmax >= 0) {
            const float xmin = (float)rmin, xmax = (float)rmax, ymin = (float)cmin, ymax = (float)cmax;
            cx = 0.5f * (xmax + xmin);
            cy = 0.5f * (ymax + ymin);
            sz = fmaxf(xmax - xmin, ymax - ymin);
        } else if (empty_fltmax) {   // Eigen-3.3 identities: centre finite (0,0), size -inf -> 100
            cx = 0.f; cy = 0.f; sz = 100.f;
        } else {                     // +-inf identities: NaN centre -> (160,160); size -> 100
            cx = 160.f; cy = 160.f; sz = 100.f;
        }
        center[b * 2 + 0] = cx;
        center[b * 2 + 1] = cy;
        if (crop_size) crop_size[b] = sz;
        const float best = sz * 1.25f;                       // nets/ColorHandPose3DNetwork.py:84
        scale[b] = fminf(fmaxf(256.0f / best, 0.25f), 5.0f);  // :85
        if (seed_out) { seed_out[b * 2] = sy; seed_out[b * 2 + 1] = sx; }
    }
}

// word wx of row y of the packed detmap (d = the image's [H,W] bytes): pixel wx * 32 + k is bit k; wx == WW is the row's zero guard word
__device__ __forceinline__ unsigned pack_det_word(const unsigned char* d, int y, int wx, int W, int WW) {
    unsigned bits = 0;
    const unsigned char* row = d + (size_t)y * W + wx * 32;
    if (wx == WW) {
        // guard word
    } else if (wx * 32 + 32 <= W && ((W & 7) == 0)) {          // 4 aligned 8-byte loads instead of 32 byte loads
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const unsigned long long v = *(const unsigned long long*)(row + q * 8);
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if ((v >> (8 * k)) & 0xffull) bits |= (1u << (q * 8 + k));
        }
    } else {
        for (int k = 0; k < 32; ++k) {
            const int x = wx * 32 + k;
            if (x < W && row[k]) bits |= (1u << k);
        }
    }
    return bits;
}

constexpr int MG_R = 12;          // rows per thread in the vertical pass of mask_grow
HP3D_KERNEL(1024)
void mask_grow_kernel(const unsigned char* det, const unsigned long long* keys, int H, int W, int empty_fltmax,
                      float* mask_out, float* center, float* crop_size, float* scale, int* seed_out) {
    HP3D_DYN_SMEM(smem_f);
    const int WW = (W + 31) >> 5, P = WW + 1;
    const int NWORD = H * P;                     // words of a bitmap incl. the guard column
    unsigned* detb = (unsigned*)smem_f;
    unsigned* obj = detb + NWORD + 1;            // obj[-1] and obj[NWORD] exist and stay zero (neighbours of the first / last word)
    unsigned* tmp = obj + NWORD + 1;
    __shared__ int s_changed[2], s_rmin, s_rmax, s_cmin, s_cmax;

    const int b = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
    const unsigned char* d = det + (size_t)b * H * W;
    const unsigned idx = 0xFFFFFFFFu - (unsigned)(keys[b] & 0xFFFFFFFFull);
    const int sy = (int)(idx / (unsigned)W), sx = (int)(idx % (unsigned)W);

    for (int w = tid; w < NWORD; w += nthr) {
        const int y = w / P, wx = w - y * P;
        detb[w] = pack_det_word(d, y, wx, W, WW);
        obj[w] = (y == sy && wx == (sx >> 5)) ? (1u << (sx & 31)) : 0u;
    }
    if (tid == 0) { s_rmin = 0x7fffffff; s_rmax = -1; s_cmin = 0x7fffffff; s_cmax = -1; s_changed[0] = s_changed[1] = 0; obj[-1] = 0u; obj[NWORD] = 0u; }
    __syncthreads();

    // this thread's first unit of the vertical pass (MG_R rows of one word column), computed once; images beyond 1024 units pay the division
    const int nseg = (H + MG_R - 1) / MG_R, nunits = nseg * WW;
    const int u0seg = tid / WW, u0wx = tid - u0seg * WW;
    const int num_passes = max(H, W) / 10;   // max(s[1], s[2]) // (filter_size // 2)
    for (int pass = 0; pass < num_passes; ++pass) {
        // horizontal dilation, radius 10: three independent LDS reads; the guard words make the row ends (their own results are never read)
        for (int w = tid; w < NWORD; w += nthr) {
            const unsigned long long lo = obj[w - 1], mid = obj[w], hi = obj[w + 1];
            unsigned long long win = (mid << 16) | (lo >> 16) | (hi << 48);
            win = win | (win << 1) | (win >> 1);     // radius 1
            win = win | (win << 2) | (win >> 2);     // radius 3
            win = win | (win << 4) | (win >> 4);     // radius 7
            win = win | (win << 3) | (win >> 3);     // radius 10
            tmp[w] = (unsigned)(win >> 16);
        }
        __syncthreads();
        // (two "changed" flags, one barrier saved per pass: the other parity's flag is cleared HERE -- every thread has read it for the
        //  previous pass's exit test before it arrived at the barrier above, and its next writers come after the next two barriers)
        if (tid == 0) s_changed[(pass + 1) & 1] = 0;
        // vertical dilation, radius 10, AND det.  A thread owns MG_R consecutive rows of one word column: it reads the
        // MG_R + 20 rows it needs once and forms the 21-row ORs by doubling (2, 4, 8, 16 rows, then 16 + 4 + 1), ~10 ORs and
        // 2.7 LDS reads per output instead of 21 + 21
        int changed = 0;
        for (int u = tid, k = 0; u < nunits; u += nthr, ++k) {
            int seg = u0seg, wx = u0wx;
            if (k) { seg = u / WW; wx = u - seg * WW; }
            const int y0 = seg * MG_R;
            unsigned v[MG_R + 20];
            // all MG_R + 20 reads are issued unconditionally (rows outside the image read the unit's own first word and are
            // masked to zero afterwards): no branches, no serialised waits
            const int base = (y0 - 10) * P + wx;
#pragma unroll
            for (int i = 0; i < MG_R + 20; ++i) {
                const bool ok = (unsigned)(y0 - 10 + i) < (unsigned)H;
                const unsigned r = tmp[ok ? base + i * P : wx];
                v[i] = ok ? r : 0u;
            }
            unsigned a2[MG_R + 17], a4[MG_R + 5];
            {
                unsigned a1[MG_R + 19];
#pragma unroll
                for (int i = 0; i < MG_R + 19; ++i) a1[i] = v[i] | v[i + 1];
#pragma unroll
                for (int i = 0; i < MG_R + 17; ++i) a2[i] = a1[i] | a1[i + 2];
                unsigned a3[MG_R + 13];
#pragma unroll
                for (int i = 0; i < MG_R + 13; ++i) a3[i] = a2[i] | a2[i + 4];
#pragma unroll
                for (int i = 0; i < MG_R + 5; ++i) a4[i] = a3[i] | a3[i + 8];
            }
#pragma unroll
            for (int j = 0; j < MG_R; ++j) {
                const int y = y0 + j;
                if (y < H) {
                    const int w = y * P + wx;
                    const unsigned acc = (a4[j] | a2[j + 16] | v[j + 20]) & detb[w];     // rows y-10 .. y+10
                    if (acc != obj[w]) changed = 1;
                    // obj is only read through tmp in this phase -> safe to update in place (its guard words are never written)
                    obj[w] = acc;
                }
            }
        }
        if (changed) s_changed[pass & 1] = 1;
        __syncthreads();
        if (!s_changed[pass & 1]) break;
    }

    // bounding box (calc_center_bb): "x" = row index, "y" = column index
    int rmin = 0x7fffffff, rmax = -1, cmin = 0x7fffffff, cmax = -1;
    for (int w = tid; w < NWORD; w += nthr) {
        const unsigned v = obj[w];
        if (v) {
            const int y = w / P, wx = w - y * P;
            rmin = min(rmin, y); rmax = max(rmax, y);
            cmin = min(cmin, wx * 32 + (__ffs(v) - 1));
            cmax = max(cmax, wx * 32 + (31 - __clz(v)));
        }
    }
    if (rmax >= 0) {
        atomicMin(&s_rmin, rmin); atomicMax(&s_rmax, rmax);
        atomicMin(&s_cmin, cmin); atomicMax(&s_cmax, cmax);
    }
    __syncthreads();
    mask_grow_epilogue(obj, P, b, H, W, s_rmin, s_rmax, s_cmin, s_cmax, sy, sx, empty_fltmax, mask_out, center, crop_size, scale, seed_out);
}

// ---------------------------------------------------------------------------------------
// The same growth for frames whose three bitmaps do not fit one workgroup's LDS (mask_grow_lds_bytes > 159 KB: 540x960 and up).
// The bitmaps (same layout: pitch P = WW + 1 with the zero guard word) live in a per-image block of global scratch,
// mask_grow_global_words(H, W) words: det, then obj with its two end guards, then tmp.  mask_pack_kernel fills det and O_0 over the
// whole chip; mask_grow_global_kernel then runs the passes with one workgroup per image.  One image's maps (0.8 MB at 1080x1920) stay
// in the L2 of the XCD the workgroup runs on.
//
// Active window (exact): O_j is zero outside its bounding box [r0,r1] x [c0,c1], so dilate(O_j) -- and with it O_{j+1} -- is zero
// outside that box grown by 10 pixels.  A pass therefore forms the horizontal dilation in rows r0..r1 only (zero elsewhere: those rows
// of obj are empty) and writes obj only on the word columns and rows of the grown box; every word outside it already holds zero in
// O_j and in O_{j+1}, so the scratch holds exactly O_{j+1} after the pass.  The box of O_{j+1} is collected from the words the pass
// writes (LDS min / max atomics, as the bounding-box epilogue), so the epilogue needs no scan.  A hand a few hundred pixels across costs
// what it costs at 320x320, whatever the frame size; the worst case is det all ones (the window spans the frame after max(H,W)/20 passes).
//
// Visibility: every word a pass reads was written by another wave of the SAME workgroup before a __syncthreads().  __syncthreads() is a
// workgroup-scope release fence (each wave waits for its stores: s_waitcnt vmcnt(0)), s_barrier, and a workgroup-scope acquire fence;
// the waves of a workgroup share one CU and its vector L1 (no threadgroup split mode here), so the AMDGPU memory model needs no cache
// invalidate at that scope and the loads after the barrier see the stores before it.  No data crosses workgroups: the pack kernel's
// stores reach this kernel through the kernel boundary on the same stream.
HP3D_KERNEL(256)
void mask_pack_kernel(const unsigned char* det, const unsigned long long* keys, int H, int W, unsigned* scratch) {
    const int WW = (W + 31) >> 5, P = WW + 1, NWORD = H * P;
    const int b = blockIdx.y;
    unsigned* detb = scratch + (size_t)b * (3 * (size_t)NWORD + 2);
    unsigned* obj = detb + NWORD + 1;
    const unsigned char* d = det + (size_t)b * H * W;
    const unsigned idx = 0xFFFFFFFFu - (unsigned)(keys[b] & 0xFFFFFFFFull);
    const int sy = (int)(idx / (unsigned)W), sx = (int)(idx % (unsigned)W);
    for (int w = blockIdx.x * blockDim.x + threadIdx.x; w < NWORD; w += gridDim.x * blockDim.x) {
        const int y = w / P, wx = w - y * P;
        detb[w] = pack_det_word(d, y, wx, W, WW);
        obj[w] = (y == sy && wx == (sx >> 5)) ? (1u << (sx & 31)) : 0u;
        if (w == 0) { obj[-1] = 0u; obj[NWORD] = 0u; }
    }
}

HP3D_KERNEL(1024)
void mask_grow_global_kernel(const unsigned long long* keys, int H, int W, int empty_fltmax, unsigned* scratch,
                             float* mask_out, float* center, float* crop_size, float* scale, int* seed_out) {
    const int WW = (W + 31) >> 5, P = WW + 1;
    const int NWORD = H * P;
    const int b = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
    const unsigned* detb = scratch + (size_t)b * (3 * (size_t)NWORD + 2);
    unsigned* obj = (unsigned*)detb + NWORD + 1;
    unsigned* tmp = obj + NWORD + 1;
    // s_box[k] = {rmin, rmax, cmin, cmax} of O_j, k = j & 1 (O_j's box is read at the top of pass j, O_{j+1}'s collected in it)
    __shared__ int s_box[2][4], s_changed[2];
    const unsigned idx = 0xFFFFFFFFu - (unsigned)(keys[b] & 0xFFFFFFFFull);
    const int sy = (int)(idx / (unsigned)W), sx = (int)(idx % (unsigned)W);
    if (tid == 0) {
        s_box[0][0] = s_box[0][1] = sy; s_box[0][2] = s_box[0][3] = sx;     // O_0 = {seed}
        if ((unsigned)sy >= (unsigned)H) s_box[0][1] = -1;                  // (no valid seed: nothing grows; the window never leaves the map)
        s_changed[0] = s_changed[1] = 0;
    }
    __syncthreads();

    const int num_passes = max(H, W) / 10;   // max(s[1], s[2]) // (filter_size // 2)
    int cur = 0;                             // s_box[cur] = the box of what obj holds
    for (int pass = 0; pass < num_passes; ++pass) {
        const int r0 = s_box[cur][0], r1 = s_box[cur][1], c0 = s_box[cur][2], c1 = s_box[cur][3];
        // (the next box's slot was last read at the top of the previous pass, before two barriers)
        if (tid == 0) { s_box[cur ^ 1][0] = 0x7fffffff; s_box[cur ^ 1][1] = -1; s_box[cur ^ 1][2] = 0x7fffffff; s_box[cur ^ 1][3] = -1; }
        if (r1 < 0) break;                   // O_j empty: so is every later one (uniform: all threads read the same box)
        const int R0 = max(r0 - 10, 0), R1 = min(r1 + 10, H - 1);
        const int wx0 = max(c0 - 10, 0) >> 5, wx1 = min(c1 + 10, W - 1) >> 5, nwx = wx1 - wx0 + 1;
        // horizontal dilation, radius 10, rows r0..r1 of the window's word columns (the guard words make the row ends)
        const int nh = (r1 - r0 + 1) * nwx;
        for (int i = tid; i < nh; i += nthr) {
            const int yy = i / nwx, w = (r0 + yy) * P + wx0 + (i - yy * nwx);
            const unsigned long long lo = obj[w - 1], mid = obj[w], hi = obj[w + 1];
            unsigned long long win = (mid << 16) | (lo >> 16) | (hi << 48);
            win = win | (win << 1) | (win >> 1);     // radius 1
            win = win | (win << 2) | (win >> 2);     // radius 3
            win = win | (win << 4) | (win >> 4);     // radius 7
            win = win | (win << 3) | (win >> 3);     // radius 10
            tmp[w] = (unsigned)(win >> 16);
        }
        __syncthreads();
        if (tid == 0) s_changed[(pass + 1) & 1] = 0;
        // vertical dilation, radius 10, AND det, rows R0..R1: as in mask_grow_kernel, MG_R rows of one word column per unit; tmp rows
        // outside r0..r1 (the rows written above) are zero
        int changed = 0;
        int rmin = 0x7fffffff, rmax = -1, cmin = 0x7fffffff, cmax = -1;
        const int nunits = ((R1 - R0 + MG_R) / MG_R) * nwx;
        for (int u = tid; u < nunits; u += nthr) {
            const int seg = u / nwx, wx = wx0 + (u - seg * nwx);
            const int y0 = R0 + seg * MG_R;
            unsigned v[MG_R + 20];
            const int base = (y0 - 10) * P + wx;
#pragma unroll
            for (int i = 0; i < MG_R + 20; ++i) {
                const int y = y0 - 10 + i;
                v[i] = (y >= r0 && y <= r1) ? tmp[base + i * P] : 0u;
            }
            unsigned a2[MG_R + 17], a4[MG_R + 5];
            {
                unsigned a1[MG_R + 19];
#pragma unroll
                for (int i = 0; i < MG_R + 19; ++i) a1[i] = v[i] | v[i + 1];
#pragma unroll
                for (int i = 0; i < MG_R + 17; ++i) a2[i] = a1[i] | a1[i + 2];
                unsigned a3[MG_R + 13];
#pragma unroll
                for (int i = 0; i < MG_R + 13; ++i) a3[i] = a2[i] | a2[i + 4];
#pragma unroll
                for (int i = 0; i < MG_R + 5; ++i) a4[i] = a3[i] | a3[i + 8];
            }
#pragma unroll
            for (int j = 0; j < MG_R; ++j) {
                const int y = y0 + j;
                if (y <= R1) {
                    const int w = y * P + wx;
                    const unsigned acc = (a4[j] | a2[j + 16] | v[j + 20]) & detb[w];     // rows y-10 .. y+10
                    if (acc != obj[w]) changed = 1;
                    obj[w] = acc;
                    if (acc) {
                        rmin = min(rmin, y); rmax = max(rmax, y);
                        cmin = min(cmin, wx * 32 + (__ffs(acc) - 1));
                        cmax = max(cmax, wx * 32 + (31 - __clz(acc)));
                    }
                }
            }
        }
        if (rmax >= 0) {
            atomicMin(&s_box[cur ^ 1][0], rmin); atomicMax(&s_box[cur ^ 1][1], rmax);
            atomicMin(&s_box[cur ^ 1][2], cmin); atomicMax(&s_box[cur ^ 1][3], cmax);
        }
        if (changed) s_changed[pass & 1] = 1;
        __syncthreads();
        cur ^= 1;
        if (!s_changed[pass & 1]) break;
    }
    mask_grow_epilogue(obj, P, b, H, W, s_box[cur][0], s_box[cur][1], s_box[cur][2], s_box[cur][3], sy, sx, empty_fltmax, mask_out,
                       center, crop_size, scale, seed_out);
}

// ---------------------------------------------------------------------------------------
// Up to K hands per image.  R_0 = det; a growth runs inside R from the first arg-max of fg over R's pixels and is then
// taken out of R (R &= ~O), so the objects are pairwise disjoint; an object of at least min_area pixels becomes the next hand, in the
// order of discovery; at most 4 K growths per image.  Slot j of image b is index b * K + j of every output.  The first seed is the image's
// global arg-max (keys): it lies in det unless det is empty, and then slot 0 is what the single-hand kernels give (empty mask, fall-back
// box) with valid = 0.  Slots that stay without a hand: valid = 0, area = 0, zero mask, seed (-1, -1), the fall-back box.
// The two kernels stand beside the single-hand ones (same passes, same bits for slot 0) instead of sharing their loop bodies, so that the
// single-hand path compiles to what it compiled to before.
//
// u64 maximum over the workgroup, returned to every thread.  Every thread calls it.
__device__ __forceinline__ unsigned long long block_max_u64_all(unsigned long long v) {
    __shared__ unsigned long long s_red[16];
    v = wave_max_u64(v);
    const int wave = threadIdx.x >> 6, nwave = (blockDim.x + 63) >> 6;
    __syncthreads();                     // (the previous call's readers are done with s_red)
    if ((threadIdx.x & 63) == 0) s_red[wave] = v;
    __syncthreads();
    for (int i = 0; i < nwave; ++i) v = s_red[i] > v ? s_red[i] : v;
    return v;
}

// the key (softmax_det_key's) of the first arg-max of fg over the set bits of the packed map R (pitch P); 0: R is empty
__device__ __forceinline__ unsigned long long mask_argmax_in(const unsigned* R, const float* fg, int W, int P, int NWORD) {
    unsigned long long best = 0ull;
    for (int w = threadIdx.x; w < NWORD; w += blockDim.x) {
        unsigned v = R[w];
        if (v) {
            const int y = w / P, wx = w - y * P;
            const unsigned base = (unsigned)y * (unsigned)W + (unsigned)wx * 32u;
            while (v) {
                const unsigned idx = base + (unsigned)(__ffs(v) - 1);
                v &= v - 1u;
                const unsigned long long key = ((unsigned long long)__float_as_uint(fg[idx]) << 32) | (unsigned long long)(0xFFFFFFFFu - idx);
                best = key > best ? key : best;
            }
        }
    }
    return block_max_u64_all(best);
}

// slot `slot` holds no hand.  Every thread of the workgroup calls it.
__device__ __forceinline__ void mask_absent_slot(int slot, int H, int W, int empty_fltmax, float* mask_out, float* center, float* crop_size,
                                                 float* scale, int* seed_out, int* valid, int* area) {
    if (mask_out) {
        float* mo = mask_out + (size_t)slot * H * W;
        for (int i = threadIdx.x; i < H * W; i += blockDim.x) mo[i] = 0.f;
    }
    mask_grow_epilogue(nullptr, 0, slot, H, W, 0x7fffffff, -1, 0x7fffffff, -1, -1, -1, empty_fltmax, nullptr, center, crop_size, scale,
                       seed_out);
    if (threadIdx.x == 0) { valid[slot] = 0; area[slot] = 0; }
}

// Kept slots: on a multi-hand tracker's detect step slot j of image b with keep[b * K + j] != 0 still follows its hand
// with the box (kc, ks); an object one of them claims is that hand, found again, and is dropped.  keep == nullptr: no kept slot.
constexpr int MG_MAXK = 4;       // = HP3D_MAX_HANDS (include/hp3d.h)
// The claim test, float32 op by op (a comparison with a NaN is false): the object's box centre (calc_center_bb's) lies within the
// slot's crop window -- half = 128 / scale pixels around its centre -- or the slot's centre lies inside the object's bounding box.
__device__ __forceinline__ bool mask_claims(float crow, float ccol, float s, int rmin, int rmax, int cmin, int cmax) {
    const float orow = 0.5f * ((float)rmax + (float)rmin), ocol = 0.5f * ((float)cmax + (float)cmin);
    const float half = 128.0f / s;
    const bool near = fabsf(orow - crow) <= half && fabsf(ocol - ccol) <= half;
    const bool inside = (float)rmin <= crow && crow <= (float)rmax && (float)cmin <= ccol && ccol <= (float)cmax;
    return near || inside;
}
// the lowest kept slot of image b that claims the object, -1: none.  The same for every thread of the workgroup.
__device__ __forceinline__ int mask_claimed_by(const int* keep, const float* kc, const float* ks, int b, int K, int rmin, int rmax, int cmin,
                                               int cmax) {
    if (!keep || rmax < 0) return -1;
    for (int j = 0; j < K; ++j) {
        const int slot = b * K + j;
        if (keep[slot] && mask_claims(kc[slot * 2], kc[slot * 2 + 1], ks[slot], rmin, rmax, cmin, cmax)) return j;
    }
    return -1;
}
__device__ __forceinline__ int mask_count_kept(const int* keep, int b, int K) {
    int n = 0;
    if (keep) for (int j = 0; j < K; ++j) n += keep[b * K + j] ? 1 : 0;
    return n;
}
// the k-th free (not kept) slot of image b, in ascending order: accepted objects go to the lowest free slot first
__device__ __forceinline__ int mask_free_slot(const int* keep, int b, int K, int k) {
    if (!keep) return k;
    for (int j = 0; j < K; ++j)
        if (!keep[b * K + j] && k-- == 0) return j;
    return K - 1;     // (not reached: the loops stop at the last free slot)
}
// The end of both multi-hand kernels: kept slots and the free slots behind the k filled ones come back absent; the claim counters.
// Every thread of the workgroup calls it.
__device__ __forceinline__ void mask_multi_finish(const int* keep, int b, int K, int k, const int* ncl, int H, int W, int empty_fltmax,
                                                  float* mask_out, float* center, float* crop_size, float* scale, int* seed_out, int* valid,
                                                  int* area, int* claimed) {
    int nfree = 0;
    for (int j = 0; j < K; ++j) {
        const bool kept = keep && keep[b * K + j];
        if (kept || nfree++ >= k) mask_absent_slot(b * K + j, H, W, empty_fltmax, mask_out, center, crop_size, scale, seed_out, valid, area);
        if (claimed && threadIdx.x == 0) claimed[b * K + j] = ncl[j];
    }
}

HP3D_KERNEL(1024)
void mask_grow_multi_kernel(const unsigned char* det, const float* fg, const unsigned long long* keys, int H, int W, int K, int min_area,
                            int empty_fltmax, float* mask_out, float* center, float* crop_size, float* scale, int* seed_out,
                            int* valid, int* area, const int* keep, const float* keep_center, const float* keep_scale, int* claimed) {
    HP3D_DYN_SMEM(smem_f);
    const int WW = (W + 31) >> 5, P = WW + 1;
    const int NWORD = H * P;
    unsigned* detb = (unsigned*)smem_f;          // R: the part of det no object has taken yet
    unsigned* obj = detb + NWORD + 1;
    unsigned* tmp = obj + NWORD + 1;
    __shared__ int s_changed[2], s_rmin, s_rmax, s_cmin, s_cmax, s_area;

    const int b = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
    const unsigned char* d = det + (size_t)b * H * W;
    const float* f = fg + (size_t)b * H * W;
    const unsigned idx0 = 0xFFFFFFFFu - (unsigned)(keys[b] & 0xFFFFFFFFull);
    int sy = (int)(idx0 / (unsigned)W), sx = (int)(idx0 % (unsigned)W);

    for (int w = tid; w < NWORD; w += nthr) {
        const int y = w / P, wx = w - y * P;
        detb[w] = pack_det_word(d, y, wx, W, WW);
    }
    if (tid == 0) { obj[-1] = 0u; obj[NWORD] = 0u; }
    __syncthreads();
    // det is empty (the global arg-max lies outside it): slot 0 is the single-hand kernel's result
    const bool empty = !((unsigned)sy < (unsigned)H && ((detb[sy * P + (sx >> 5)] >> (sx & 31)) & 1u));
    // with kept slots an empty det leaves every free slot absent: nothing is grown
    const int nkept = mask_count_kept(keep, b, K), nfree = K - nkept;
    const bool legacy = empty && nkept == 0;
    int ncl[MG_MAXK] = {0, 0, 0, 0};

    const int nseg = (H + MG_R - 1) / MG_R, nunits = nseg * WW;
    const int num_passes = max(H, W) / 10;   // max(s[1], s[2]) // (filter_size // 2)
    int k = 0, tries = 0;
    for (; legacy || !empty;) {
        for (int w = tid; w < NWORD; w += nthr) {
            const int y = w / P, wx = w - y * P;
            obj[w] = (y == sy && wx == (sx >> 5)) ? (1u << (sx & 31)) : 0u;
        }
        if (tid == 0) { s_rmin = 0x7fffffff; s_rmax = -1; s_cmin = 0x7fffffff; s_cmax = -1; s_area = 0; s_changed[0] = s_changed[1] = 0; }
        __syncthreads();
        for (int pass = 0; pass < num_passes; ++pass) {         // the passes of mask_grow_kernel, inside R
            for (int w = tid; w < NWORD; w += nthr) {
                const unsigned long long lo = obj[w - 1], mid = obj[w], hi = obj[w + 1];
                unsigned long long win = (mid << 16) | (lo >> 16) | (hi << 48);
                win = win | (win << 1) | (win >> 1);     // radius 1
                win = win | (win << 2) | (win >> 2);     // radius 3
                win = win | (win << 4) | (win >> 4);     // radius 7
                win = win | (win << 3) | (win >> 3);     // radius 10
                tmp[w] = (unsigned)(win >> 16);
            }
            __syncthreads();
            if (tid == 0) s_changed[(pass + 1) & 1] = 0;
            int changed = 0;
            for (int u = tid; u < nunits; u += nthr) {
                const int seg = u / WW, wx = u - seg * WW;
                const int y0 = seg * MG_R;
                unsigned v[MG_R + 20];
                const int base = (y0 - 10) * P + wx;
#pragma unroll
                for (int i = 0; i < MG_R + 20; ++i) {
                    const bool ok = (unsigned)(y0 - 10 + i) < (unsigned)H;
                    const unsigned r = tmp[ok ? base + i * P : wx];
                    v[i] = ok ? r : 0u;
                }
                unsigned a2[MG_R + 17], a4[MG_R + 5];
                {
                    unsigned a1[MG_R + 19];
#pragma unroll
                    for (int i = 0; i < MG_R + 19; ++i) a1[i] = v[i] | v[i + 1];
#pragma unroll
                    for (int i = 0; i < MG_R + 17; ++i) a2[i] = a1[i] | a1[i + 2];
                    unsigned a3[MG_R + 13];
#pragma unroll
                    for (int i = 0; i < MG_R + 13; ++i) a3[i] = a2[i] | a2[i + 4];
#pragma unroll
                    for (int i = 0; i < MG_R + 5; ++i) a4[i] = a3[i] | a3[i + 8];
                }
#pragma unroll
                for (int j = 0; j < MG_R; ++j) {
                    const int y = y0 + j;
                    if (y < H) {
                        const int w = y * P + wx;
                        const unsigned acc = (a4[j] | a2[j + 16] | v[j + 20]) & detb[w];     // rows y-10 .. y+10
                        if (acc != obj[w]) changed = 1;
                        obj[w] = acc;
                    }
                }
            }
            if (changed) s_changed[pass & 1] = 1;
            __syncthreads();
            if (!s_changed[pass & 1]) break;
        }
        // bounding box and pixel count of the object
        int rmin = 0x7fffffff, rmax = -1, cmin = 0x7fffffff, cmax = -1, cnt = 0;
        for (int w = tid; w < NWORD; w += nthr) {
            const unsigned v = obj[w];
            if (v) {
                const int y = w / P, wx = w - y * P;
                rmin = min(rmin, y); rmax = max(rmax, y);
                cmin = min(cmin, wx * 32 + (__ffs(v) - 1));
                cmax = max(cmax, wx * 32 + (31 - __clz(v)));
                cnt += __builtin_popcount(v);
            }
        }
        if (rmax >= 0) {
            atomicMin(&s_rmin, rmin); atomicMax(&s_rmax, rmax);
            atomicMin(&s_cmin, cmin); atomicMax(&s_cmax, cmax);
            atomicAdd(&s_area, cnt);
        }
        __syncthreads();
        const int obj_area = s_area, rmin_o = s_rmin, rmax_o = s_rmax, cmin_o = s_cmin, cmax_o = s_cmax;
        const int claim = mask_claimed_by(keep, keep_center, keep_scale, b, K, rmin_o, rmax_o, cmin_o, cmax_o);
        // a claimed object is dropped whatever its area; with no free slot (all kept) the others are dropped as well
        const bool accept = claim < 0 && k < nfree && (legacy || obj_area >= min_area);
        if (claim >= 0) ++ncl[claim];
        if (accept) {
            const int slot = b * K + mask_free_slot(keep, b, K, k);
            mask_grow_epilogue(obj, P, slot, H, W, rmin_o, rmax_o, cmin_o, cmax_o, sy, sx, empty_fltmax, mask_out, center, crop_size, scale,
                               seed_out);
            if (tid == 0) { valid[slot] = legacy ? 0 : 1; area[slot] = obj_area; }
            ++k;
        }
        for (int w = tid; w < NWORD; w += nthr) detb[w] &= ~obj[w];
        ++tries;
        if (legacy || (accept && k == nfree) || tries == 4 * K) break;
        __syncthreads();        // R is final; the box and obj have been read
        const unsigned long long key = mask_argmax_in(detb, f, W, P, NWORD);
        if (!key) break;        // nothing left
        const unsigned idx = 0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull);
        sy = (int)(idx / (unsigned)W); sx = (int)(idx % (unsigned)W);
    }
    mask_multi_finish(keep, b, K, k, ncl, H, W, empty_fltmax, mask_out, center, crop_size, scale, seed_out, valid, area, claimed);
}

// The same on the per-image scratch block of mask_grow_global_kernel (mask_pack_kernel has filled det and set the first seed).  The
// active window restarts at each seed: a finished object is taken out of R and cleared from obj on its own bounding box, so obj is zero
// outside the new seed again and the exactness argument above holds per growth (rows of tmp outside the window are never read).
HP3D_KERNEL(1024)
void mask_grow_multi_global_kernel(const float* fg, const unsigned long long* keys, int H, int W, int K, int min_area, int empty_fltmax,
                                   unsigned* scratch, float* mask_out, float* center, float* crop_size, float* scale, int* seed_out,
                                   int* valid, int* area, const int* keep, const float* keep_center, const float* keep_scale, int* claimed) {
    const int WW = (W + 31) >> 5, P = WW + 1;
    const int NWORD = H * P;
    const int b = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
    unsigned* detb = scratch + (size_t)b * (3 * (size_t)NWORD + 2);      // R
    unsigned* obj = detb + NWORD + 1;
    unsigned* tmp = obj + NWORD + 1;
    const float* f = fg + (size_t)b * H * W;
    __shared__ int s_box[2][4], s_changed[2], s_area;
    const unsigned idx0 = 0xFFFFFFFFu - (unsigned)(keys[b] & 0xFFFFFFFFull);
    int sy = (int)(idx0 / (unsigned)W), sx = (int)(idx0 % (unsigned)W);
    const bool seed_ok = (unsigned)sy < (unsigned)H;
    const bool empty = !(seed_ok && ((detb[sy * P + (sx >> 5)] >> (sx & 31)) & 1u));
    const int nkept = mask_count_kept(keep, b, K), nfree = K - nkept;
    const bool legacy = empty && nkept == 0;
    int ncl[MG_MAXK] = {0, 0, 0, 0};

    const int num_passes = max(H, W) / 10;   // max(s[1], s[2]) // (filter_size // 2)
    int k = 0, tries = 0;
    for (; legacy || !empty;) {
        if (tid == 0) {
            s_box[0][0] = s_box[0][1] = sy; s_box[0][2] = s_box[0][3] = sx;     // O_0 = {seed}
            if (!seed_ok) s_box[0][1] = -1;
            else obj[sy * P + (sx >> 5)] = 1u << (sx & 31);
            s_changed[0] = s_changed[1] = 0; s_area = 0;
        }
        __syncthreads();
        int cur = 0;                             // s_box[cur] = the box of what obj holds
        for (int pass = 0; pass < num_passes; ++pass) {         // the passes of mask_grow_global_kernel, inside R
            const int r0 = s_box[cur][0], r1 = s_box[cur][1], c0 = s_box[cur][2], c1 = s_box[cur][3];
            if (tid == 0) { s_box[cur ^ 1][0] = 0x7fffffff; s_box[cur ^ 1][1] = -1; s_box[cur ^ 1][2] = 0x7fffffff; s_box[cur ^ 1][3] = -1; }
            if (r1 < 0) break;
            const int R0 = max(r0 - 10, 0), R1 = min(r1 + 10, H - 1);
            const int wx0 = max(c0 - 10, 0) >> 5, wx1 = min(c1 + 10, W - 1) >> 5, nwx = wx1 - wx0 + 1;
            const int nh = (r1 - r0 + 1) * nwx;
            for (int i = tid; i < nh; i += nthr) {
                const int yy = i / nwx, w = (r0 + yy) * P + wx0 + (i - yy * nwx);
                const unsigned long long lo = obj[w - 1], mid = obj[w], hi = obj[w + 1];
                unsigned long long win = (mid << 16) | (lo >> 16) | (hi << 48);
                win = win | (win << 1) | (win >> 1);     // radius 1
                win = win | (win << 2) | (win >> 2);     // radius 3
                win = win | (win << 4) | (win >> 4);     // radius 7
                win = win | (win << 3) | (win >> 3);     // radius 10
                tmp[w] = (unsigned)(win >> 16);
            }
            __syncthreads();
            if (tid == 0) s_changed[(pass + 1) & 1] = 0;
            int changed = 0;
            int rmin = 0x7fffffff, rmax = -1, cmin = 0x7fffffff, cmax = -1;
            const int nunits = ((R1 - R0 + MG_R) / MG_R) * nwx;
            for (int u = tid; u < nunits; u += nthr) {
                const int seg = u / nwx, wx = wx0 + (u - seg * nwx);
                const int y0 = R0 + seg * MG_R;
                unsigned v[MG_R + 20];
                const int base = (y0 - 10) * P + wx;
#pragma unroll
                for (int i = 0; i < MG_R + 20; ++i) {
                    const int y = y0 - 10 + i;
                    v[i] = (y >= r0 && y <= r1) ? tmp[base + i * P] : 0u;
                }
                unsigned a2[MG_R + 17], a4[MG_R + 5];
                {
                    unsigned a1[MG_R + 19];
#pragma unroll
                    for (int i = 0; i < MG_R + 19; ++i) a1[i] = v[i] | v[i + 1];
#pragma unroll
                    for (int i = 0; i < MG_R + 17; ++i) a2[i] = a1[i] | a1[i + 2];
                    unsigned a3[MG_R + 13];
#pragma unroll
                    for (int i = 0; i < MG_R + 13; ++i) a3[i] = a2[i] | a2[i + 4];
#pragma unroll
                    for (int i = 0; i < MG_R + 5; ++i) a4[i] = a3[i] | a3[i + 8];
                }
#pragma unroll
                for (int j = 0; j < MG_R; ++j) {
                    const int y = y0 + j;
                    if (y <= R1) {
                        const int w = y * P + wx;
                        const unsigned acc = (a4[j] | a2[j + 16] | v[j + 20]) & detb[w];     // rows y-10 .. y+10
                        if (acc != obj[w]) changed = 1;
                        obj[w] = acc;
                        if (acc) {
                            rmin = min(rmin, y); rmax = max(rmax, y);
                            cmin = min(cmin, wx * 32 + (__ffs(acc) - 1));
                            cmax = max(cmax, wx * 32 + (31 - __clz(acc)));
                        }
                    }
                }
            }
            if (rmax >= 0) {
                atomicMin(&s_box[cur ^ 1][0], rmin); atomicMax(&s_box[cur ^ 1][1], rmax);
                atomicMin(&s_box[cur ^ 1][2], cmin); atomicMax(&s_box[cur ^ 1][3], cmax);
            }
            if (changed) s_changed[pass & 1] = 1;
            __syncthreads();
            cur ^= 1;
            if (!s_changed[pass & 1]) break;
        }
        // pixel count over the object's box (obj is zero outside it)
        const int r0 = s_box[cur][0], r1 = s_box[cur][1], c0 = s_box[cur][2], c1 = s_box[cur][3];
        const int bw0 = r1 >= 0 ? (c0 >> 5) : 0, nbw = r1 >= 0 ? (c1 >> 5) - bw0 + 1 : 0, nbox = r1 >= 0 ? (r1 - r0 + 1) * nbw : 0;
        int cnt = 0;
        for (int i = tid; i < nbox; i += nthr) {
            const int yy = i / nbw;
            cnt += __builtin_popcount(obj[(r0 + yy) * P + bw0 + (i - yy * nbw)]);
        }
        if (cnt) atomicAdd(&s_area, cnt);
        __syncthreads();
        const int obj_area = s_area;
        const int claim = mask_claimed_by(keep, keep_center, keep_scale, b, K, r0, r1, c0, c1);
        const bool accept = claim < 0 && k < nfree && (legacy || obj_area >= min_area);
        if (claim >= 0) ++ncl[claim];
        if (accept) {
            const int slot = b * K + mask_free_slot(keep, b, K, k);
            mask_grow_epilogue(obj, P, slot, H, W, r0, r1, c0, c1, sy, sx, empty_fltmax, mask_out, center, crop_size, scale, seed_out);
            if (tid == 0) { valid[slot] = legacy ? 0 : 1; area[slot] = obj_area; }
            ++k;
        }
        __syncthreads();        // the mask has been read from obj
        for (int i = tid; i < nbox; i += nthr) {
            const int yy = i / nbw, w = (r0 + yy) * P + bw0 + (i - yy * nbw);
            detb[w] &= ~obj[w];
            obj[w] = 0u;
        }
        ++tries;
        if (legacy || (accept && k == nfree) || tries == 4 * K) break;
        __syncthreads();        // R is final, obj is zero
        const unsigned long long key = mask_argmax_in(detb, f, W, P, NWORD);
        if (!key) break;        // nothing left
        const unsigned idx = 0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull);
        sy = (int)(idx / (unsigned)W); sx = (int)(idx % (unsigned)W);
    }
    mask_multi_finish(keep, b, K, k, ncl, H, W, empty_fltmax, mask_out, center, crop_size, scale, seed_out, valid, area, claimed);
}

// ---------------------------------------------------------------------------------------
// Fully connected: out[b][o] = sum_i x[b][i] * W[i][o] + bias[o]  (utils/general.py:112-136)
// Weight-streaming bound (4-9 MB of weights, a few MFLOP): split-K over many workgroups so the whole
// chip streams W once, then a fixed-order reduction (deterministic, no atomics).
//   pass 1: workgroup = 64 outputs x one 128-row K slice x up to 32 batch rows; 4 K-quarters per
//           workgroup, x slice staged transposed in LDS, W rows read coalesced (256 B per row).
//   pass 2: out = act(bias + sum over K slices in index order).
constexpr int FC_KCH = 128, FC_BT = 32;
// x = [x | x2]: columns 0..F1-1 come from x (row stride x_stride), columns F1..Cin-1 from x2 (row stride Cin - F1) -- the
// concat([flatten, hand_side]) of nets/ColorHandPose3DNetwork.py:262-263,297-298 without a copy (x2 = nullptr, F1 = Cin: plain).
// The thread's 32 weights are all requested BEFORE the first multiply-add (round 5: the loop used to load one weight per
// iteration behind a data-dependent exit, 32 dependent HBM / L2 round trips per workgroup = 12-25 us per launch for a few
// MFLOP; the sums are the same, in the same order: rows beyond Cin contribute fmaf(0, 0, acc) = acc).
// conv_s (round 6): 0 = a plain matrix x; S > 0 = the rows are the OUTPUT PIXELS of a 3x3 / stride-2 / SAME convolution of an [n,S,S,conv_c] map (S even:
// TensorFlow pads 0 before, 1 after), row = (image, oy, ox), column gk = (tap r * 3 + s) * conv_c + c -- i.e. the layer's HWIO filter IS the FC
// matrix.  The lifting towers' last stride-2 layers (8x8 -> 4x4 maps: 512 output pixels at B = 32) run here: as implicit GEMMs on 8x8-pixel tiles
// they were the slowest launches of the stage (ViewpointNet/conv_vp_2_2 47 us at 12.8 TFLOP/s).
HP3D_KERNEL(256)
void fc_partial_kernel(const float* x, int B, int Cin, int x_stride, const float* x2, int F1, const float* w, int Cout, float* part, int conv_s, int conv_c) {
    __shared__ float xs[FC_KCH][FC_BT + 4];        // [k][b], pitch 36 floats (16-B aligned rows)
    __shared__ float red[4][FC_BT][64];
    const int o = blockIdx.x * 64 + (threadIdx.x & 63);
    const int kq = threadIdx.x >> 6;               // K quarter: rows kq*32 .. kq*32+31 of the slice
    const int k0 = blockIdx.y * FC_KCH;
    const int b0 = blockIdx.z * FC_BT;
    float wv[32];
#pragma unroll
    for (int u = 0; u < 32; ++u) {
        const int gk = k0 + kq * 32 + u;
        wv[u] = (o < Cout && gk < Cin) ? w[(size_t)gk * Cout + o] : 0.f;
    }
    for (int i = threadIdx.x; i < FC_KCH * FC_BT; i += 256) {
        const int b = i / FC_KCH, kk = i - b * FC_KCH;       // coalesced along k
        const int gb = b0 + b, gk = k0 + kk;
        float v = 0.f;
        if (conv_s) {
            if (gb < B && gk < Cin) {
                const int so = conv_s >> 1, img = gb / (so * so), op = gb - img * so * so, oy = op / so, ox = op - oy * so;
                const int tap = gk / conv_c, c = gk - tap * conv_c, iy = 2 * oy + tap / 3, ix = 2 * ox + tap % 3;
                if (iy < conv_s && ix < conv_s) v = x[((size_t)(img * conv_s + iy) * conv_s + ix) * conv_c + c];
            }
        } else if (gb < B && gk < Cin) v = gk < F1 ? x[(size_t)gb * x_stride + gk] : x2[(size_t)gb * (Cin - F1) + (gk - F1)];
        xs[kk][b] = v;
    }
    __syncthreads();
    float acc[FC_BT];
#pragma unroll
    for (int j = 0; j < FC_BT; ++j) acc[j] = 0.f;
#pragma unroll
    for (int u = 0; u < 32; ++u) {
        const int kk = kq * 32 + u;
#pragma unroll
        for (int j4 = 0; j4 < FC_BT / 4; ++j4) {
            const f32x4 xv = *(const f32x4*)&xs[kk][j4 * 4];
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[j4 * 4 + e] = fmaf(xv[e], wv[u], acc[j4 * 4 + e]);
        }
    }
#pragma unroll
    for (int j = 0; j < FC_BT; ++j) red[kq][j][threadIdx.x & 63] = acc[j];
    __syncthreads();
    // 256 threads reduce the 4 quarters for 32 x 64 outputs
    for (int i = threadIdx.x; i < FC_BT * 64; i += 256) {
        const int j = i >> 6, oo = i & 63;
        const int gb = b0 + j, go = blockIdx.x * 64 + oo;
        if (gb < B && go < Cout)
            part[((size_t)blockIdx.y * B + gb) * Cout + go] = (red[0][j][oo] + red[1][j][oo]) + (red[2][j][oo] + red[3][j][oo]);
    }
}

HP3D_KERNEL(256)
void fc_reduce_kernel(const float* part, int nslices, int B, int Cout, const float* bias, int act, float* out,
                      int out_stride) {
    const int total = B * Cout;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int b = i / Cout, o = i - b * Cout;
        // the slices are added in index order (deterministic); eight loads are in flight at a time -- one load per addition is a chain of
        // nslices (17 / 33) dependent memory round trips, 12-23 us for a few KB (round 5)
        float v = 0.f;
        int s = 0;
        for (; s + 8 <= nslices; s += 8) {
            float t[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) t[u] = part[((size_t)(s + u) * B + b) * Cout + o];
#pragma unroll
            for (int u = 0; u < 8; ++u) v += t[u];
        }
        for (; s < nslices; ++s) v += part[((size_t)s * B + b) * Cout + o];
        v += bias[o];
        if (act) v = leaky(v);
        out[(size_t)b * out_stride + o] = v;
    }
}

// The tail of a lifting tower as ONE launch (round 6): the fixed-order reduction of the first FC layer's K slices (+ bias, leaky-ReLU), then the two small
// FC layers behind it (PosePrior: 512 -> 512 -> 63, nets/ColorHandPose3DNetwork.py:264-270; ViewpointNet: 256 -> 128 -> 3, :299-307).  As
// fc_partial + fc_reduce each, those were five launches of a few microseconds of work at the launch floor (18-20 us per layer); here a workgroup
// takes FCT_G images through all three steps with the activations in LDS.  Layer 1: thread = (4 consecutive outputs, one K part), the parts added in
// index order; layer 2: thread = (image, output).  Deterministic.
constexpr int FCT_G = 2, FCT_MAXC = 512;
HP3D_KERNEL(256)
void fc_tail_kernel(const float* part0, int ns0, int B, int C0, const float* bias0, int act0, const float* w1, const float* b1, int C1, int act1,
                    const float* w2, const float* b2, int C2, int act2, float* out, int out_stride) {
    __shared__ __attribute__((aligned(16))) float h0[FCT_G][FCT_MAXC];
    __shared__ __attribute__((aligned(16))) float h1[FCT_G][FCT_MAXC];
    __shared__ __attribute__((aligned(16))) float red[8 * FCT_G * 128];          // [K part][image][C1] (C1 * parts = 1024)
    const int tid = threadIdx.x, img0 = blockIdx.x * FCT_G;
    // layer 0: the K slices in index order (what fc_reduce_kernel does), eight loads in flight
    for (int i = tid; i < FCT_G * C0; i += 256) {
        const int g = i / C0, o = i - g * C0, gb = img0 + g;
        float v = 0.f;
        if (gb < B) {
            int sl = 0;
            for (; sl + 8 <= ns0; sl += 8) {
                float t[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) t[u] = part0[((size_t)(sl + u) * B + gb) * C0 + o];
#pragma unroll
                for (int u = 0; u < 8; ++u) v += t[u];
            }
            for (; sl < ns0; ++sl) v += part0[((size_t)sl * B + gb) * C0 + o];
            v += bias0[o];
            if (act0) v = leaky(v);
        }
        h0[g][o] = v;
    }
    __syncthreads();
    // layer 1: C1 / 4 threads cover the outputs, 256 / (C1 / 4) K parts
    {
        const int no4 = C1 >> 2, kp = 256 / no4, o4 = (tid % no4) * 4, part = tid / no4;
        const int klen = (C0 + kp - 1) / kp, k0 = part * klen, k1 = min(C0, k0 + klen);
        f32x4 acc[FCT_G];
#pragma unroll
        for (int g = 0; g < FCT_G; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (part < kp) {
            int k = k0;
            for (; k + 8 <= k1; k += 8) {
                f32x4 wv[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) wv[u] = *(const f32x4*)(w1 + (size_t)(k + u) * C1 + o4);
#pragma unroll
                for (int u = 0; u < 8; ++u)
#pragma unroll
                    for (int g = 0; g < FCT_G; ++g) {
                        const float xv = h0[g][k + u];
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[g][e] = fmaf(xv, wv[u][e], acc[g][e]);
                    }
            }
            for (; k < k1; ++k) {
                const f32x4 wv = *(const f32x4*)(w1 + (size_t)k * C1 + o4);
#pragma unroll
                for (int g = 0; g < FCT_G; ++g)
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[g][e] = fmaf(h0[g][k], wv[e], acc[g][e]);
            }
#pragma unroll
            for (int g = 0; g < FCT_G; ++g) *(f32x4*)&red[(part * FCT_G + g) * C1 + o4] = acc[g];
        }
        __syncthreads();
        for (int i = tid; i < FCT_G * C1; i += 256) {
            const int g = i / C1, o = i - g * C1;
            float v = 0.f;
            for (int pp = 0; pp < kp; ++pp) v += red[(pp * FCT_G + g) * C1 + o];
            v += b1[o];
            if (act1) v = leaky(v);
            h1[g][o] = v;
        }
    }
    __syncthreads();
    // layer 2 (63 / 3 outputs): thread = (image, output), the K loop in index order
    for (int i = tid; i < FCT_G * C2; i += 256) {
        const int g = i / C2, o = i - g * C2, gb = img0 + g;
        if (gb >= B) continue;
        float v = 0.f;
        int k = 0;
        for (; k + 8 <= C1; k += 8) {
            float wv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) wv[u] = w2[(size_t)(k + u) * C2 + o];
#pragma unroll
            for (int u = 0; u < 8; ++u) v = fmaf(h1[g][k + u], wv[u], v);
        }
        for (; k < C1; ++k) v = fmaf(h1[g][k], w2[(size_t)k * C2 + o], v);
        v += b2[o];
        if (act2) v = leaky(v);
        out[(size_t)gb * out_stride + o] = v;
    }
}

// _get_rot_mat + _flip_right_hand + matmul (nets/ColorHandPose3DNetwork.py:240-245,311-334)
HP3D_KERNEL(64)
void lift_epilogue_kernel(const float* u, const float* can, const float* hand_side, int B, float* rot,
                          float* rel, int do_rot) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    float R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (do_rot) {
        const float ux_b = u[b * 3], uy_b = u[b * 3 + 1], uz_b = u[b * 3 + 2];
        const float un = sqrtf(((ux_b * ux_b + uy_b * uy_b) + uz_b * uz_b) + 1e-8f);
        const float st = sinf(un), ct = cosf(un), oc = 1.0f - ct;
        const float nf = 1.0f / un;
        const float ux = ux_b * nf, uy = uy_b * nf, uz = uz_b * nf;
        R[0] = ct + ux * ux * oc; R[1] = ux * uy * oc - uz * st; R[2] = ux * uz * oc + uy * st;
        R[3] = uy * ux * oc + uz * st; R[4] = ct + uy * uy * oc; R[5] = uy * uz * oc - ux * st;
        R[6] = uz * ux * oc - uy * st; R[7] = uz * uy * oc + ux * st; R[8] = ct + uz * uz * oc;
        if (rot) for (int i = 0; i < 9; ++i) rot[b * 9 + i] = R[i];
    }
    const bool right = do_rot && (hand_side[b * 2 + 1] > hand_side[b * 2]);   // argmax(hand_side)==1
    for (int k = 0; k < 21; ++k) {
        const float x = can[b * 63 + k * 3], y = can[b * 63 + k * 3 + 1];
        const float z = right ? -can[b * 63 + k * 3 + 2] : can[b * 63 + k * 3 + 2];
        for (int j = 0; j < 3; ++j) rel[b * 63 + k * 3 + j] = (x * R[j] + y * R[3 + j]) + z * R[6 + j];
    }
}

// bone_rel_trafo_inv (utils/relative_trafo.py:243-295; PosePriorNetwork variants 'local*',
// nets/PosePriorNetwork.py:70-75).  One thread per image walks the 5 finger chains root -> tip.
// The chain transform T (global -> bone frame) is rigid, T = [R | t], so the reference's
//   T_new = Trans_z(-len) * RotX(-ax) * RotY(-ay) * T_parent ;  x = matrix_inverse(T_new) * (0,0,0,1)^T
// is evaluated as R_new = M R, t_new = M t + (0,0,-len), x = -R_new^T t_new  (M = RotX(-ax) RotY(-ay)).
HP3D_KERNEL(64)
void bone_rel_inv_kernel(const float* rel, int B, float* xyz) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int chains[6][4] = {{0, -1, -1, -1}, {4, 3, 2, 1}, {8, 7, 6, 5}, {12, 11, 10, 9}, {16, 15, 14, 13}, {20, 19, 18, 17}};
    for (int ci = 0; ci < 6; ++ci) {
        float R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, tv[3] = {0, 0, 0};
        for (int k = 0; k < 4; ++k) {
            const int bone = chains[ci][k];
            if (bone < 0) break;
            const float len = rel[b * 63 + bone * 3], ax = -rel[b * 63 + bone * 3 + 1], ay = -rel[b * 63 + bone * 3 + 2];
            const float cx = cosf(ax), sx = sinf(ax), cy = cosf(ay), sy = sinf(ay);
            // M = RotX(ax) * RotY(ay), RotX = [1 0 0; 0 c -s; 0 s c], RotY = [c 0 s; 0 1 0; -s 0 c]
            const float M[9] = {cy, 0.f, sy, sx * sy, cx, -sx * cy, -cx * sy, sx, cx * cy};
            float Rn[9], tn[3];
            for (int i = 0; i < 3; ++i) {
                for (int j = 0; j < 3; ++j) Rn[i * 3 + j] = (M[i * 3] * R[j] + M[i * 3 + 1] * R[3 + j]) + M[i * 3 + 2] * R[6 + j];
                tn[i] = (M[i * 3] * tv[0] + M[i * 3 + 1] * tv[1]) + M[i * 3 + 2] * tv[2];
            }
            tn[2] -= len;
            for (int i = 0; i < 9; ++i) R[i] = Rn[i];
            for (int i = 0; i < 3; ++i) tv[i] = tn[i];
            for (int j = 0; j < 3; ++j) xyz[b * 63 + bone * 3 + j] = -((R[j] * tv[0] + R[3 + j] * tv[1]) + R[6 + j] * tv[2]);
        }
    }
}

// detect_keypoints (utils/general.py:331-344): first arg-max per channel; one workgroup per (b,c)
// order-preserving key of a float for np.argmax's ordering: -0.0 and +0.0 are equal (the first one wins), and a NaN beats
// everything (np.argmax returns the first NaN)
__device__ __forceinline__ unsigned ord_f32(float f) {
    unsigned u = __float_as_uint(f);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return 0xFFFFFFFFu;       // NaN, either sign
    if ((u & 0x7FFFFFFFu) == 0u) u = 0u;                           // -0.0 -> +0.0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
HP3D_KERNEL(256)
void argmax2d_kernel(const float* x, int H, int W, int C, int cs, int* out_rc) {
    __shared__ unsigned long long red[4];
    const int c = blockIdx.x, b = blockIdx.y;
    const float* xb = x + (size_t)b * H * W * cs + c;
    unsigned long long best = 0ull;
    for (int i = threadIdx.x; i < H * W; i += blockDim.x) {
        const unsigned long long key = ((unsigned long long)ord_f32(xb[(size_t)i * cs]) << 32) |
                                       (unsigned long long)(0xFFFFFFFFu - (unsigned)i);
        best = key > best ? key : best;
    }
    best = wave_max_u64(best);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 4; ++i) best = red[i] > best ? red[i] : best;
        const unsigned idx = 0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFull);
        out_rc[((size_t)b * C + c) * 2] = (int)(idx / (unsigned)W);
        out_rc[((size_t)b * C + c) * 2 + 1] = (int)(idx % (unsigned)W);
    }
}

// detect_keypoints + trafo_coords (utils/general.py:331-357) WITHOUT the 256 x 256 x 21 map in HBM: one workgroup per
// (channel, image) holds the h x w score map of its channel in LDS, evaluates tf.image.resize_images' arithmetic
// (resize_bilinear_kernel above, op for op) for every pixel of the oh x ow map and keeps the FIRST maximum in row-major
// order -- exactly np.argmax of the up-sampled map, ties and rounding included (the maximum of the small map times the
// up-sampling factor is NOT always it: a neighbour 1 ulp below the peak can round up to the peak value at an earlier
// interpolated position).  kp_crop [B,C,2] int32 (row, col); kp_image [B,C,2] float64 =
// (kp - crop_size // 2) / scale + center evaluated in double like NumPy does on float64 keypoints and float32 scale / centre.
HP3D_KERNEL(256)
void kp_detect_kernel(const float* sm, int h, int w, int C, int cs, int oh, int ow, const float* scale,
                      const float* center, int* kp_crop, double* kp_image) {
    __shared__ float src[64 * 64];
    __shared__ unsigned long long red[4];
    const int c = blockIdx.x, b = blockIdx.y;
    const float* xb = sm + (size_t)b * h * w * cs + c;
    for (int i = threadIdx.x; i < h * w; i += blockDim.x) src[i] = xb[(size_t)i * cs];
    __syncthreads();
    const float hscale = (float)h / (float)oh, wscale = (float)w / (float)ow;
    unsigned long long best = 0ull;
    for (int oy = threadIdx.x; oy < oh; oy += blockDim.x) {
        int y0, y1; float ty;
        resize_coord(oy, hscale, h, y0, y1, ty);
        for (int ox = 0; ox < ow; ++ox) {
            int x0, x1; float tx;
            resize_coord(ox, wscale, w, x0, x1, tx);
            const float tl = src[y0 * w + x0], tr = src[y0 * w + x1], bl = src[y1 * w + x0], br = src[y1 * w + x1];
            const float top = tl + (tr - tl) * tx;
            const float bot = bl + (br - bl) * tx;
            const float v = top + (bot - top) * ty;
            const unsigned long long key = ((unsigned long long)ord_f32(v) << 32) |
                                           (unsigned long long)(0xFFFFFFFFu - (unsigned)(oy * ow + ox));
            best = key > best ? key : best;
        }
    }
    best = wave_max_u64(best);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < 4; ++i) best = red[i] > best ? red[i] : best;
        const unsigned idx = 0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFull);
        const int row = (int)(idx / (unsigned)ow), col = (int)(idx % (unsigned)ow);
        const size_t o = ((size_t)b * C + c) * 2;
        if (kp_crop) { kp_crop[o] = row; kp_crop[o + 1] = col; }
        if (kp_image) {
            const double sc = (double)scale[b];
            kp_image[o] = ((double)row - (double)(oh / 2)) / sc + (double)center[b * 2];
            kp_image[o + 1] = ((double)col - (double)(ow / 2)) / sc + (double)center[b * 2 + 1];
        }
    }
}

// ---- tracking ----------------------------------------------------------------------------------------
// np.maximum / np.minimum: a NaN on either side is the result (fmaxf / fminf would drop it, and the rule below relies on it reaching
// the "not finite -> 200" test)
__device__ __forceinline__ float np_maximum(float a, float b) { return (a >= b || a != a) ? a : b; }
__device__ __forceinline__ float np_minimum(float a, float b) { return (a <= b || a != a) ? a : b; }
__device__ __forceinline__ bool finite_f32(float f) { return (__float_as_uint(f) & 0x7F800000u) != 0x7F800000u; }

// The next frame's crop box from this frame's 21 image-space keypoints: the dataset readers' hand_crop rule
// (data/BinaryDbReader.py:268-308, data/BinaryDbReaderSTB.py:219-259), float32 op by op in the reader's order, all 21 keypoints
// "visible": centre = keypoint 12 ((0, 0) when not finite), size = 2 x the largest distance from the centre to the keypoints'
// bounding box clamped to the frame, x margin, clamped to [50, 500] (not finite -> 200), scale = crop / size clamped to [1, 10].
// margin = 1 is the reader's rule bit for bit; 1.25 is the factor the detection path puts on its own box (ColorHandPose3DNetwork.py:84).
// One workgroup per image.  kp_image [B,21,2] float64 (row, col) as kp_detect_kernel writes it; sm (may be null) the last 32 x 32
// score maps with channel stride cs: confidence = mean over the 21 channels (added in channel order) of each channel's maximum
// (NaNs never win), 0 without a map.  lost = 1 when keypoint 12 is not finite or lies outside the frame (row < 0, row > H, col < 0,
// col > W), or -- with a threshold and a map -- when the confidence is not at least the threshold.
struct TrackBox { float cy, cx, scale, conf; int lost; };
// Every thread of the (256-thread) workgroup calls it; the result is thread 0's.
__device__ __forceinline__ TrackBox track_box_rule(const double* kp_image, const float* sm, int cs, int b, int H, int W, int crop, float margin,
                                                   float min_score, int use_min_score) {
    __shared__ float cmax[256];
    const int t = threadIdx.x;
    TrackBox r = {0.f, 0.f, 1.f, 0.f, 0};
    if (sm) {
        const int c = t & 31, g = t >> 5;
        float m = -__builtin_inff();
        if (c < 21) {
            const float* xb = sm + (size_t)b * 1024 * cs + c;
            for (int i = g; i < 1024; i += 8) {
                const float v = xb[(size_t)i * cs];
                m = v > m ? v : m;
            }
        }
        cmax[t] = m;
    }
    __syncthreads();
    if (t == 0) {
        float conf = 0.f;
        if (sm) {
            float s = 0.f;
            for (int c = 0; c < 21; ++c) {
                float m = cmax[c];
                for (int g = 1; g < 8; ++g) m = cmax[g * 32 + c] > m ? cmax[g * 32 + c] : m;
                s = s + m;
            }
            conf = s / 21.0f;
        }
        const double* kp = kp_image + (size_t)b * 42;
        const float r12 = (float)kp[24], c12 = (float)kp[25];
        const bool cfin = finite_f32(r12) && finite_f32(c12);
        const float cy = cfin ? r12 : 0.f, cx = cfin ? c12 : 0.f;
        float mn0 = (float)kp[0], mn1 = (float)kp[1], mx0 = mn0, mx1 = mn1;
        for (int k = 1; k < 21; ++k) {
            const float r = (float)kp[k * 2], c = (float)kp[k * 2 + 1];
            mn0 = np_minimum(mn0, r); mn1 = np_minimum(mn1, c);
            mx0 = np_maximum(mx0, r); mx1 = np_maximum(mx1, c);
        }
        mn0 = np_maximum(mn0, 0.f); mn1 = np_maximum(mn1, 0.f);
        mx0 = np_minimum(mx0, (float)H); mx1 = np_minimum(mx1, (float)W);
        const float b0 = 2.f * np_maximum(mx0 - cy, cy - mn0), b1 = 2.f * np_maximum(mx1 - cx, cx - mn1);
        float best = np_maximum(b0, b1);
        best = best * margin;
        best = np_minimum(np_maximum(best, 50.f), 500.f);
        if (!finite_f32(best)) best = 200.f;
        r.cy = cy; r.cx = cx;
        r.scale = np_minimum(np_maximum((float)crop / best, 1.f), 10.f);
        r.conf = conf;
        r.lost = (!cfin || r12 < 0.f || r12 > (float)H || c12 < 0.f || c12 > (float)W ||
                  (use_min_score && sm && !(conf >= min_score))) ? 1 : 0;
    }
    return r;
}

// detected0 (may be null): zeroed for the image (a tracked step's "no box of this step came from HandSegNet").
HP3D_KERNEL(256)
void track_box_kernel(const double* kp_image, const float* sm, int cs, int H, int W, int crop, float margin, float min_score,
                      int use_min_score, float* center, float* scale, float* confidence, int* lost, int* detected0) {
    const int b = blockIdx.x;
    const TrackBox r = track_box_rule(kp_image, sm, cs, b, H, W, crop, margin, min_score, use_min_score);
    if (threadIdx.x == 0) {
        center[b * 2] = r.cy; center[b * 2 + 1] = r.cx;
        scale[b] = r.scale;
        confidence[b] = r.conf;
        lost[b] = r.lost;
        if (detected0) detected0[b] = 0;
    }
}

// The same per slot of the multi-hand tracker, one workgroup per slot: a slot that holds a hand (valid != 0) gets
// track_box_kernel's box and `lost`; an absent slot holds the box it cropped with (box_center / box_scale: its fall-back box) and
// lost = 0; the confidence is reported for both.  keep_next (may be null) = valid and not lost: the slots a detect step behind this
// step keeps.  detected0 / area0 / claimed0 (may be null): zeroed (a tracked step).
HP3D_KERNEL(256)
void track_hands_box_kernel(const double* kp_image, const float* sm, int cs, int H, int W, int crop, float margin, float min_score,
                            int use_min_score, const int* valid, const float* box_center, const float* box_scale, float* center,
                            float* scale, float* confidence, int* lost, int* keep_next, int* detected0, int* area0, int* claimed0) {
    const int b = blockIdx.x;
    const TrackBox r = track_box_rule(kp_image, sm, cs, b, H, W, crop, margin, min_score, use_min_score);
    if (threadIdx.x == 0) {
        const bool v = valid[b] != 0;
        center[b * 2] = v ? r.cy : box_center[b * 2];
        center[b * 2 + 1] = v ? r.cx : box_center[b * 2 + 1];
        scale[b] = v ? r.scale : box_scale[b];
        confidence[b] = r.conf;
        lost[b] = v ? r.lost : 0;
        if (keep_next) keep_next[b] = (v && !r.lost) ? 1 : 0;
        if (detected0) detected0[b] = 0;
        if (area0) area0[b] = 0;
        if (claimed0) claimed0[b] = 0;
    }
}

// A multi-hand detect step's choice per slot: a kept slot holds its tracked box (detected = 0, valid = 1, area = 0); any other takes what
// the claimed growth wrote for it -- a newly found hand (detected = valid = 1, its box and pixel count) or nothing (valid = 0, area = 0,
// the fall-back box).
HP3D_KERNEL(256)
void track_hands_select_kernel(const int* keep, const float* det_center, const float* det_scale, const int* det_valid, const int* det_area,
                               int n, float* box_center, float* box_scale, int* valid, int* detected, int* area) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        if (keep[i]) {
            valid[i] = 1; detected[i] = 0; area[i] = 0;
        } else {
            const int v = det_valid[i] != 0 ? 1 : 0;
            box_center[i * 2] = det_center[i * 2]; box_center[i * 2 + 1] = det_center[i * 2 + 1];
            box_scale[i] = det_scale[i];
            valid[i] = v; detected[i] = v; area[i] = v ? det_area[i] : 0;
        }
    }
}

// A detect step's choice per image: an image whose previous box was lost (or every image, force_all) takes HandSegNet's box,
// the others keep the tracked one.  detected[b] = 1 where HandSegNet's was taken.
HP3D_KERNEL(256)
void track_select_kernel(const int* lost_prev, const float* det_center, const float* det_scale, int B, int force_all,
                         float* box_center, float* box_scale, int* detected) {
    for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < B; b += gridDim.x * blockDim.x) {
        const int d = (force_all || lost_prev[b] != 0) ? 1 : 0;
        if (d) {
            box_center[b * 2] = det_center[b * 2]; box_center[b * 2 + 1] = det_center[b * 2 + 1];
            box_scale[b] = det_scale[b];
        }
        detected[b] = d;
    }
}

// ---- detection on a reduced frame (option "detect_scale" = f) -------------------------------------------------------
// The detection frame: pixel (y, x, c) of the [Hd, Wd] = [ceil(H / f), ceil(W / f)] output is the mean of the source window rows
// [y f, min((y + 1) f, H)) x columns [x f, min((x + 1) f, W)) -- clipped, n = the real count.  float32 frames: the window added in
// row-major order as a sequential float32 sum, then / float(n).  uint8 frames: the exact integer sum, then (float(sum) / float(n)) / 255
// - 0.5 in preprocess_u8_kernel's order; the normalised full-size frame never exists.
// One thread takes one output pixel with its 3 channels: a window row is f * 3 contiguous elements, the rows of neighbouring lanes lie
// side by side (a wave reads 64 f * 3 contiguous elements of a frame row per load), the 3 floats written per lane likewise.  F > 0
// (f = 2, 4, 8 with `wide`: frame base and row pitch multiples of ALIGN bytes): a full window row is ONE load of F * 3 elements at
// the widest alignment the pixel size allows -- 8 / 16 / 16 bytes for float32, 2 / 4 / 8 bytes for uint8 (3 bytes per pixel: a window
// row starts on a 16-byte boundary only every fourth window at f = 4) -- instead of F * 3 element loads.
template <typename T> struct DownAcc { typedef float type; };
template <> struct DownAcc<unsigned char> { typedef unsigned type; };
__device__ __forceinline__ float downscale_finish(float sum, float n) { return sum / n; }
__device__ __forceinline__ float downscale_finish(unsigned sum, float n) { return ((float)sum / n) / 255.0f - 0.5f; }
// IDX (option "track_partial_detect"): output frame b is built from source frame idx[b] -- B = the number of output frames.
// A frame is H row pitches long, so where the base and the row pitch are multiples of ALIGN (`wide`) every selected frame's base is one too.
template <typename T, int F, bool IDX = false>
__device__ __forceinline__ void downscale_body(const T* img, int B, int H, int W, int f, int Hd, int Wd, int wide, float* out,
                                               const int* idx = nullptr) {
    typedef typename DownAcc<T>::type acc_t;
    constexpr int NV = F > 0 ? F * 3 : 1;
    constexpr int ROWB = NV * (int)sizeof(T);
    constexpr int ALIGN = ROWB % 16 == 0 ? 16 : ROWB % 8 == 0 ? 8 : ROWB % 4 == 0 ? 4 : ROWB % 2 == 0 ? 2 : 1;
    const long total = (long)B * Hd * Wd;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int x = (int)(i % Wd);
        long r = i / Wd;
        const int y = (int)(r % Hd);
        const int b = (int)(r / Hd);
        const int y0 = y * f, y1 = min(y0 + f, H), x0 = x * f, nx = min(x0 + f, W) - x0;
        acc_t s0 = 0, s1 = 0, s2 = 0;
        const int sb = IDX ? idx[b] : b;
        const T* p = img + (((size_t)sb * H + y0) * W + x0) * 3;
        for (int yy = y0; yy < y1; ++yy, p += (size_t)W * 3) {
            if (F > 0 && wide && nx == F) {
                T v[NV];
                __builtin_memcpy(v, __builtin_assume_aligned(p, ALIGN), sizeof(v));
#pragma unroll
                for (int k = 0; k < NV; k += 3) { s0 += v[k]; s1 += v[k + 1]; s2 += v[k + 2]; }
            } else {
                for (int k = 0; k < nx * 3; k += 3) { s0 += p[k]; s1 += p[k + 1]; s2 += p[k + 2]; }
            }
        }
        const float n = (float)((y1 - y0) * nx);
        float* o = out + (size_t)i * 3;
        o[0] = downscale_finish(s0, n); o[1] = downscale_finish(s1, n); o[2] = downscale_finish(s2, n);
    }
}
template <int F>
HP3D_KERNEL(256)
void downscale_kernel(const float* img, int B, int H, int W, int f, int Hd, int Wd, int wide, float* out) {
    downscale_body<float, F>(img, B, H, W, f, Hd, Wd, wide, out);
}
template <int F>
HP3D_KERNEL(256)
void downscale_u8_kernel(const unsigned char* img, int B, int H, int W, int f, int Hd, int Wd, int wide, float* out) {
    downscale_body<unsigned char, F>(img, B, H, W, f, Hd, Wd, wide, out);
}
template <int F>
HP3D_KERNEL(256)
void downscale_idx_kernel(const float* img, const int* idx, int m, int H, int W, int f, int Hd, int Wd, int wide, float* out) {
    downscale_body<float, F, true>(img, m, H, W, f, Hd, Wd, wide, out, idx);
}
template <int F>
HP3D_KERNEL(256)
void downscale_u8_idx_kernel(const unsigned char* img, const int* idx, int m, int H, int W, int f, int Hd, int Wd, int wide, float* out) {
    downscale_body<unsigned char, F, true>(img, m, H, W, f, Hd, Wd, wide, out, idx);
}

// The detection frame of NV12 frames: every luma pixel of the window is converted (the clamp and the floor make the rule
// non-linear: the mean of the converted pixels is not the conversion of the mean), the three integer sums are exact, the finish is the
// uint8 frames' -- downscale_u8 on the converted frame bit for bit.  F > 0 (f = 2, 4, 8 with `wide`: both plane bases, the pitch and the
// frame stride multiples of F): a full window row is ONE F-byte load of Y, and the window's chroma row -- F / 2 pairs, shared by two luma
// rows (y0 is even) -- ONE F-byte load per two luma rows.  Odd f, ragged windows and unaligned surfaces: pixel by pixel.
// the three sums of the window rows [y0, y1) x columns [x0, x0 + nx) of frame sb (also the surface kernels' NV12 branch)
template <int F>
__device__ __forceinline__ void downscale_nv12_window(const Nv12Src& P, size_t sb, int y0, int y1, int x0, int nx, int wide, unsigned& s0,
                                                      unsigned& s1, unsigned& s2) {
    constexpr int NB = F > 0 ? F : 1;
    if constexpr (F > 0) if (wide && nx == F) {
        const size_t fb = sb * P.frame_stride;
        for (int yy = y0; yy < y1; yy += 2) {          // (H and y0 are even: rows come in pairs that share a chroma row)
            unsigned char uv[NB], ya[NB], yb[NB];
            __builtin_memcpy(uv, __builtin_assume_aligned(P.uv + fb + (size_t)(yy >> 1) * P.pitch + x0, NB), NB);
            __builtin_memcpy(ya, __builtin_assume_aligned(P.y + fb + (size_t)yy * P.pitch + x0, NB), NB);
            __builtin_memcpy(yb, __builtin_assume_aligned(P.y + fb + (size_t)(yy + 1) * P.pitch + x0, NB), NB);
#pragma unroll
            for (int k = 0; k < NB; ++k) {
                const Rgb8 pa = nv12_convert(P, ya[k], uv[k & ~1], uv[k | 1]);
                const Rgb8 pb = nv12_convert(P, yb[k], uv[k & ~1], uv[k | 1]);
                s0 += pa.r + pb.r; s1 += pa.g + pb.g; s2 += pa.b + pb.b;
            }
        }
        return;
    }
    for (int yy = y0; yy < y1; ++yy)
        for (int k = 0; k < nx; ++k) {
            const Rgb8 p = nv12_pixel(P, sb, yy, x0 + k);
            s0 += p.r; s1 += p.g; s2 += p.b;
        }
}
template <int F, bool IDX>
__device__ __forceinline__ void downscale_nv12_body(const Nv12Src P, int B, int H, int W, int f, int Hd, int Wd, int wide, float* out,
                                                    const int* idx) {
    const long total = (long)B * Hd * Wd;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int x = (int)(i % Wd);
        long r = i / Wd;
        const int y = (int)(r % Hd);
        const int b = (int)(r / Hd);
        const int y0 = y * f, y1 = min(y0 + f, H), x0 = x * f, nx = min(x0 + f, W) - x0;
        const size_t sb = (size_t)(IDX ? idx[b] : b);
        unsigned s0 = 0, s1 = 0, s2 = 0;
        downscale_nv12_window<F>(P, sb, y0, y1, x0, nx, wide, s0, s1, s2);
        const float n = (float)((y1 - y0) * nx);
        float* o = out + (size_t)i * 3;
        o[0] = downscale_finish(s0, n); o[1] = downscale_finish(s1, n); o[2] = downscale_finish(s2, n);
    }
}
template <int F>
HP3D_KERNEL(256)
void downscale_nv12_kernel(const Nv12Src src, int B, int H, int W, int f, int Hd, int Wd, int wide, float* out) {
    downscale_nv12_body<F, false>(src, B, H, W, f, Hd, Wd, wide, out, nullptr);
}
template <int F>
HP3D_KERNEL(256)
void downscale_nv12_idx_kernel(const Nv12Src src, const int* idx, int m, int H, int W, int f, int Hd, int Wd, int wide, float* out) {
    downscale_nv12_body<F, true>(src, m, H, W, f, Hd, Wd, wide, out, idx);
}

// NV12 -> the normalised float32 frame (preprocess_u8 at equal sizes on the converted frame, bit for bit) and NV12 -> uint8 RGB.  One
// thread takes the two pixels of a chroma pair: one 2-byte load of Y, one of UV; output frame b comes from source frame idx[b] (IDX).
template <bool IDX>
HP3D_KERNEL(256)
void preprocess_nv12_kernel(const Nv12Src P, const int* idx, int B, int H, int W, float* out) {
    const int W2 = W / 2;
    const long total = (long)B * H * W2;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int x = (int)(i % W2) * 2;
        long r = i / W2;
        const int y = (int)(r % H);
        const int b = (int)(r / H);
        const size_t fb = (size_t)(IDX ? idx[b] : b) * P.frame_stride;
        unsigned char yy[2], uv[2];
        __builtin_memcpy(yy, P.y + fb + (size_t)y * P.pitch + x, 2);
        __builtin_memcpy(uv, P.uv + fb + (size_t)(y >> 1) * P.pitch + x, 2);
        const Rgb8 p0 = nv12_convert(P, yy[0], uv[0], uv[1]), p1 = nv12_convert(P, yy[1], uv[0], uv[1]);
        float* o = out + (((size_t)b * H + y) * W + x) * 3;
        o[0] = u8_norm(p0.r); o[1] = u8_norm(p0.g); o[2] = u8_norm(p0.b);
        o[3] = u8_norm(p1.r); o[4] = u8_norm(p1.g); o[5] = u8_norm(p1.b);
    }
}
HP3D_KERNEL(256)
void nv12_to_rgb_kernel(const Nv12Src P, int B, int H, int W, unsigned char* out) {
    const int W2 = W / 2;
    const long total = (long)B * H * W2;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int x = (int)(i % W2) * 2;
        long r = i / W2;
        const int y = (int)(r % H);
        const int b = (int)(r / H);
        const size_t fb = (size_t)b * P.frame_stride;
        unsigned char yy[2], uv[2];
        __builtin_memcpy(yy, P.y + fb + (size_t)y * P.pitch + x, 2);
        __builtin_memcpy(uv, P.uv + fb + (size_t)(y >> 1) * P.pitch + x, 2);
        const Rgb8 p0 = nv12_convert(P, yy[0], uv[0], uv[1]), p1 = nv12_convert(P, yy[1], uv[0], uv[1]);
        unsigned char* o = out + (((size_t)b * H + y) * W + x) * 3;
        o[0] = (unsigned char)p0.r; o[1] = (unsigned char)p0.g; o[2] = (unsigned char)p0.b;
        o[3] = (unsigned char)p1.r; o[4] = (unsigned char)p1.g; o[5] = (unsigned char)p1.b;
    }
}

// The detection frame of packed 8-bit frames: one thread per output pixel, three exact unsigned sums, the uint8 frames'
// finish -- downscale_u8 on the repacked frame bit for bit.  F > 0 (f = 2, 4, 8 with `wide`: base, pitch and frame stride multiples of the
// load's alignment): a full window row is F pixel_bytes bytes in the fewest loads of at most 16 bytes -- 8 / 16 / 2 x 16 bytes for 4-byte
// pixels, and for 3-byte pixels downscale_body<unsigned char, F>'s 6 / 12 / 24 bytes at 2 / 4 / 8-byte alignment, the pitch explicit.
// A full window lies inside its row, so neither reaches past it.  Odd f, ragged windows and unaligned surfaces: pixel by pixel.
// the three sums of the window rows [y0, y1) x columns [x0, x0 + nx) of frame sb (also the surface kernels' packed branch)
template <int F>
__device__ __forceinline__ void downscale_px_window(const PxSrc& P, size_t sb, int y0, int y1, int x0, int nx, int wide, unsigned& s0,
                                                    unsigned& s1, unsigned& s2) {
    constexpr int NP = F > 0 ? F : 1;
    constexpr int A4 = NP * 4 >= 16 ? 16 : NP * 4;
    constexpr int A3 = (NP * 3) % 8 == 0 ? 8 : (NP * 3) % 4 == 0 ? 4 : (NP * 3) % 2 == 0 ? 2 : 1;
    if constexpr (F > 0) if (wide && nx == F) {
        const unsigned char* p = P.px + sb * P.frame_stride + (size_t)y0 * P.pitch + (size_t)x0 * P.pixel_bytes;
        if (P.pixel_bytes == 4) {
            for (int yy = y0; yy < y1; ++yy, p += P.pitch) {
                unsigned v[NP];
                __builtin_memcpy(v, __builtin_assume_aligned(p, A4), sizeof(v));
#pragma unroll
                for (int k = 0; k < NP; ++k) {
                    const Rgb8 q = px_unpack(P, v[k]);
                    s0 += q.r; s1 += q.g; s2 += q.b;
                }
            }
        } else {          // (3-byte pixels: the sums per byte position, sorted into R, G, B once at the end)
            unsigned t0 = 0, t1 = 0, t2 = 0;
            for (int yy = y0; yy < y1; ++yy, p += P.pitch) {
                unsigned char v[NP * 3];
                __builtin_memcpy(v, __builtin_assume_aligned(p, A3), sizeof(v));
#pragma unroll
                for (int k = 0; k < NP * 3; k += 3) { t0 += v[k]; t1 += v[k + 1]; t2 += v[k + 2]; }
            }
            s0 = P.ro == 0 ? t0 : P.ro == 1 ? t1 : t2;
            s1 = P.go == 0 ? t0 : P.go == 1 ? t1 : t2;
            s2 = P.bo == 0 ? t0 : P.bo == 1 ? t1 : t2;
        }
        return;
    }
    for (int yy = y0; yy < y1; ++yy)
        for (int k = 0; k < nx; ++k) {
            const Rgb8 q = px_pixel(P, sb, yy, x0 + k);
            s0 += q.r; s1 += q.g; s2 += q.b;
        }
}
template <int F, bool IDX>
__device__ __forceinline__ void downscale_px_body(const PxSrc P, int B, int H, int W, int f, int Hd, int Wd, int wide, float* out,
                                                  const int* idx) {
    const long total = (long)B * Hd * Wd;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int x = (int)(i % Wd);
        long r = i / Wd;
        const int y = (int)(r % Hd);
        const int b = (int)(r / Hd);
        const int y0 = y * f, y1 = min(y0 + f, H), x0 = x * f, nx = min(x0 + f, W) - x0;
        const size_t sb = (size_t)(IDX ? idx[b] : b);
        unsigned s0 = 0, s1 = 0, s2 = 0;
        downscale_px_window<F>(P, sb, y0, y1, x0, nx, wide, s0, s1, s2);
        const float n = (float)((y1 - y0) * nx);
        float* o = out + (size_t)i * 3;
        o[0] = downscale_finish(s0, n); o[1] = downscale_finish(s1, n); o[2] = downscale_finish(s2, n);
    }
}
template <int F>
HP3D_KERNEL(256)
void downscale_px_kernel(const PxSrc src, int B, int H, int W, int f, int Hd, int Wd, int wide, float* out) {
    downscale_px_body<F, false>(src, B, H, W, f, Hd, Wd, wide, out, nullptr);
}
template <int F>
HP3D_KERNEL(256)
void downscale_px_idx_kernel(const PxSrc src, const int* idx, int m, int H, int W, int f, int Hd, int Wd, int wide, float* out) {
    downscale_px_body<F, true>(src, m, H, W, f, Hd, Wd, wide, out, idx);
}

// packed 8-bit -> the normalised float32 frame (preprocess_u8 at equal sizes on the repacked frame, bit for bit) and -> uint8 RGB.  One
// thread per pixel: neighbouring lanes fetch neighbouring pixels and write neighbouring triples; output frame b comes from source frame
// idx[b] (IDX).
template <bool IDX>
HP3D_KERNEL(256)
void preprocess_px_kernel(const PxSrc P, const int* idx, int B, int H, int W, float* out) {
    const long total = (long)B * H * W;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int x = (int)(i % W);
        long r = i / W;
        const int y = (int)(r % H);
        const int b = (int)(r / H);
        const Rgb8 q = px_pixel(P, (size_t)(IDX ? idx[b] : b), y, x);
        float* o = out + (size_t)i * 3;
        o[0] = u8_norm(q.r); o[1] = u8_norm(q.g); o[2] = u8_norm(q.b);
    }
}
HP3D_KERNEL(256)
void px_to_rgb_kernel(const PxSrc P, int B, int H, int W, unsigned char* out) {
    const long total = (long)B * H * W;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int x = (int)(i % W);
        long r = i / W;
        const int y = (int)(r % H);
        const int b = (int)(r / H);
        const Rgb8 q = px_pixel(P, (size_t)b, y, x);
        unsigned char* o = out + (size_t)i * 3;
        o[0] = (unsigned char)q.r; o[1] = (unsigned char)q.g; o[2] = (unsigned char)q.b;
    }
}

// ---- a batch of separate surfaces: the detection frame, the normalised frame, the uint8 RGB frame ------------------------
// One thread per output pixel, as the packed kernels: output frame b comes from record b (or idx[b]), read once per output pixel; its
// window goes through downscale_px_window / downscale_nv12_window on the one-frame view of the record, wide where THAT surface's own
// address and pitch allow it (SurfRec::dwide, bit F) -- downscale_u8 on the stacked RGB frames bit for bit on either path.  A workgroup
// may straddle two frames: the record index is per lane.
template <int F, bool IDX>
__device__ __forceinline__ void downscale_surf_body(const SurfSrc S, int B, int H, int W, int f, int Hd, int Wd, float* out, const int* idx) {
    const long total = (long)B * Hd * Wd;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int x = (int)(i % Wd);
        long r = i / Wd;
        const int y = (int)(r % Hd);
        const int b = (int)(r / Hd);
        const int y0 = y * f, y1 = min(y0 + f, H), x0 = x * f, nx = min(x0 + f, W) - x0;
        const SurfRec R = S.rec[IDX ? idx[b] : b];
        const int wide = F > 0 ? (R.dwide >> F) & 1 : 0;
        unsigned s0 = 0, s1 = 0, s2 = 0;
        if (R.nv12) downscale_nv12_window<F>(surf_nv12(S, R), 0, y0, y1, x0, nx, wide, s0, s1, s2);
        else downscale_px_window<F>(surf_px(R), 0, y0, y1, x0, nx, wide, s0, s1, s2);
        const float n = (float)((y1 - y0) * nx);
        float* o = out + (size_t)i * 3;
        o[0] = downscale_finish(s0, n); o[1] = downscale_finish(s1, n); o[2] = downscale_finish(s2, n);
    }
}
template <int F>
HP3D_KERNEL(256)
void downscale_surf_kernel(const SurfSrc src, int B, int H, int W, int f, int Hd, int Wd, float* out) {
    downscale_surf_body<F, false>(src, B, H, W, f, Hd, Wd, out, nullptr);
}
template <int F>
HP3D_KERNEL(256)
void downscale_surf_idx_kernel(const SurfSrc src, const int* idx, int m, int H, int W, int f, int Hd, int Wd, float* out) {
    downscale_surf_body<F, true>(src, m, H, W, f, Hd, Wd, out, idx);
}
template <bool IDX>
HP3D_KERNEL(256)
void preprocess_surf_kernel(const SurfSrc S, const int* idx, int B, int H, int W, float* out) {
    const long total = (long)B * H * W;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int x = (int)(i % W);
        long r = i / W;
        const int y = (int)(r % H);
        const int b = (int)(r / H);
        const SurfRec R = S.rec[IDX ? idx[b] : b];
        const Rgb8 q = surf_pixel(S, R, y, x);
        float* o = out + (size_t)i * 3;
        o[0] = u8_norm(q.r); o[1] = u8_norm(q.g); o[2] = u8_norm(q.b);
    }
}
HP3D_KERNEL(256)
void surf_to_rgb_kernel(const SurfSrc S, int B, int H, int W, unsigned char* out) {
    const long total = (long)B * H * W;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int x = (int)(i % W);
        long r = i / W;
        const int y = (int)(r % H);
        const int b = (int)(r / H);
        const SurfRec R = S.rec[b];
        const Rgb8 q = surf_pixel(S, R, y, x);
        unsigned char* o = out + (size_t)i * 3;
        o[0] = (unsigned char)q.r; o[1] = (unsigned char)q.g; o[2] = (unsigned char)q.b;
    }
}

// A detection-frame box (centre_d, crop_size_d) in frame coordinates: centre = centre_d * f + (f - 1) / 2 (the centre of detection pixel
// p covers frame pixels p f ... p f + f - 1), crop_size = crop_size_d * f, scale from it as mask_grow_epilogue derives it (NumPy's NaN
// rules: oracle.general.scale_from_crop_size).  Element by element: may run in place.
HP3D_KERNEL(256)
void box_to_frame_kernel(const float* center_d, const float* crop_size_d, int n, float ff, float off, float* center, float* crop_size,
                         float* scale) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float cy = center_d[i * 2] * ff + off, cx = center_d[i * 2 + 1] * ff + off;
        const float sz = crop_size_d[i] * ff;
        center[i * 2] = cy; center[i * 2 + 1] = cx;
        if (crop_size) crop_size[i] = sz;
        const float best = sz * 1.25f;
        scale[i] = np_minimum(np_maximum(256.0f / best, 0.25f), 5.0f);
    }
}

// The other direction for the slots a multi-hand detect step keeps: the claim rule (mask_claims) compares them with objects of the
// detection frame.  centre_d = (centre - (f - 1) / 2) / f, scale_d = scale * f (half = 128 / scale_d: the window's half side in
// detection pixels).
HP3D_KERNEL(256)
void box_to_detect_kernel(const float* center, const float* scale, int n, float ff, float off, float* center_d, float* scale_d) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        center_d[i * 2] = (center[i * 2] - off) / ff;
        center_d[i * 2 + 1] = (center[i * 2 + 1] - off) / ff;
        scale_d[i] = scale[i] * ff;
    }
}

// ---- compaction of absent hand slots (option "hands_compact") --------------------------------------------------------
// The back half of the multi-hand calls at batch m = the slots that hold a hand.  idx [m] = those slots' indices b K + j, ascending;
// pos [ns] = a slot's dense index, -1 for an absent one.  The kernels stand beside the ones they restate (crop_and_resize_body,
// track_hands_box_kernel), which compile to what they compiled to before.
//
// Dense crop i: box idx[i] of the slot-layout center / scale, cut from image idx[i] / K.  crop_and_resize_body's arithmetic op by op.
template <class Tap>
__device__ __forceinline__ void crop_and_resize_idx_body(const Tap tap, int m, int H, int W, int C, const float* center, const float* scale,
                                                         const int* idx, int K, int crop, float* out) {
    const long total = (long)m * crop * crop;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int x = (int)(i % crop);
        long r = i / crop;
        const int y = (int)(r % crop);
        const int b = idx[(int)(r / crop)];
        const float cs = (float)crop / scale[b];
        const float half = floorf(cs / 2.0f);
        float y1 = center[b * 2 + 0] - half, y2 = y1 + cs;
        float x1 = center[b * 2 + 1] - half, x2 = x1 + cs;
        y1 = y1 / (float)H; y2 = y2 / (float)H; x1 = x1 / (float)W; x2 = x2 / (float)W;
        const float hs = (crop > 1) ? (y2 - y1) * (float)(H - 1) / (float)(crop - 1) : 0.f;
        const float ws = (crop > 1) ? (x2 - x1) * (float)(W - 1) / (float)(crop - 1) : 0.f;
        const float in_y = (crop > 1) ? y1 * (float)(H - 1) + (float)y * hs : 0.5f * (y1 + y2) * (float)(H - 1);
        const float in_x = (crop > 1) ? x1 * (float)(W - 1) + (float)x * ws : 0.5f * (x1 + x2) * (float)(W - 1);
        float* o = out + (size_t)i * C;
        const bool ok = in_y >= 0.f && in_y <= (float)(H - 1) && in_x >= 0.f && in_x <= (float)(W - 1);
        if (!ok) {
            for (int c = 0; c < C; ++c) o[c] = 0.f;
            continue;
        }
        const int ty0 = (int)floorf(in_y), ty1 = (int)ceilf(in_y);
        const int tx0 = (int)floorf(in_x), tx1 = (int)ceilf(in_x);
        const float ly = in_y - (float)ty0, lx = in_x - (float)tx0;
        if constexpr (Tap::PIXEL) {
            crop_pixel_taps(tap, (size_t)(b / K), ty0, ty1, tx0, tx1, ly, lx, o);
        } else {
            const size_t ib = (size_t)(b / K) * H * W;
            for (int c = 0; c < C; ++c) {
                const float tl = tap(ib + (size_t)ty0 * W + tx0, c), tr = tap(ib + (size_t)ty0 * W + tx1, c);
                const float bl = tap(ib + (size_t)ty1 * W + tx0, c), br = tap(ib + (size_t)ty1 * W + tx1, c);
                const float top = tl + (tr - tl) * lx;
                const float bot = bl + (br - bl) * lx;
                o[c] = top + (bot - top) * ly;
            }
        }
    }
}
HP3D_KERNEL(256)
void crop_and_resize_idx_kernel(const float* img, int m, int H, int W, int C, const float* center, const float* scale, const int* idx, int K,
                                int crop, float* out) {
    crop_and_resize_idx_body(TapF32{img, C}, m, H, W, C, center, scale, idx, K, crop, out);
}
HP3D_KERNEL(256)
void crop_and_resize_idx_u8_kernel(const unsigned char* img, int m, int H, int W, const float* center, const float* scale, const int* idx,
                                   int K, int crop, float* out) {
    crop_and_resize_idx_body(TapU8{img, 3}, m, H, W, 3, center, scale, idx, K, crop, out);
}
HP3D_KERNEL(256)
void crop_and_resize_idx_nv12_kernel(const Nv12Src src, int m, int H, int W, const float* center, const float* scale, const int* idx, int K,
                                     int crop, float* out) {
    crop_and_resize_idx_body(TapNv12{src}, m, H, W, 3, center, scale, idx, K, crop, out);
}
HP3D_KERNEL(256)
void crop_and_resize_idx_px_kernel(const PxSrc src, int m, int H, int W, const float* center, const float* scale, const int* idx, int K,
                                   int crop, float* out) {
    crop_and_resize_idx_body(TapPx{src}, m, H, W, 3, center, scale, idx, K, crop, out);
}
HP3D_KERNEL(256)
void crop_and_resize_idx_surf_kernel(const SurfSrc src, int m, int H, int W, const float* center, const float* scale, const int* idx, int K,
                                     int crop, float* out) {
    crop_and_resize_idx_body(TapSurf{src}, m, H, W, 3, center, scale, idx, K, crop, out);
}

// hand_side / centre / scale of the m slots as dense arrays for the lifting stage and kp_detect: latency only
HP3D_KERNEL(256)
void slot_gather_kernel(const int* idx, int m, const float* hand_side, const float* center, const float* scale, float* hand_side_d,
                        float* center_d, float* scale_d) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) {
        const int s = idx[i];
        if (hand_side_d) { hand_side_d[i * 2] = hand_side[s * 2]; hand_side_d[i * 2 + 1] = hand_side[s * 2 + 1]; }
        if (center_d) { center_d[i * 2] = center[s * 2]; center_d[i * 2 + 1] = center[s * 2 + 1]; }
        if (scale_d) scale_d[i] = scale[s];
    }
}

// Dense results -> the caller's slot layout, absent slots filled with 0: the one bandwidth path of the compacted calls (image_crop
// 786 KB and kp_scoremap 5.5 MB per slot).  The grid lies over (segment, slot): a segment is SCATTER_SEG_WORDS consecutive words of one
// array of one slot, so a slot's copy or fill is spread over the chip; consecutive lanes take consecutive 16-byte (vec) or 4-byte words.
constexpr unsigned SCATTER_SEG_WORDS = 8192;          // 32 KB: 8 rounds of 256 lanes x 16 bytes
HP3D_KERNEL(256)
void slot_scatter_kernel(ScatterPlan plan, const int* pos, int ns) {
    int k = 0;
    for (int i = 1; i < plan.n; ++i)
        if (blockIdx.x >= plan.a[i].seg0) k = i;
    const ScatterArray A = plan.a[k];
    const unsigned w0 = (blockIdx.x - A.seg0) * SCATTER_SEG_WORDS;
    const unsigned w1 = min(w0 + SCATTER_SEG_WORDS, A.words);
    for (int slot = blockIdx.y; slot < ns; slot += gridDim.y) {
        const int p = pos[slot];
        float* d = A.dst + (size_t)slot * A.words;
        const float* sp = A.src + (size_t)(p < 0 ? 0 : p) * A.words;
        if (A.vec) {
            for (unsigned w = w0 + threadIdx.x * 4; w < w1; w += 1024) {
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (p >= 0) v = *(const f32x4*)(sp + w);
                *(f32x4*)(d + w) = v;
            }
        } else {
            // (words, not floats: an int32 or half a float64 must keep its bits)
            const unsigned* su = (const unsigned*)sp;
            unsigned* du = (unsigned*)d;
            for (unsigned w = w0 + threadIdx.x; w < w1; w += 256) du[w] = p >= 0 ? su[w] : 0u;
        }
    }
}

// track_hands_box_kernel behind a compacted back half, one workgroup per slot: kp_image / sm hold the m slots that ran.  A slot that
// ran (pos >= 0: it is valid) gets track_box_rule on its dense entry; an absent slot holds its box with lost = 0, confidence = 0.
HP3D_KERNEL(256)
void track_hands_box_pos_kernel(const double* kp_image, const float* sm, int cs, int H, int W, int crop, float margin, float min_score,
                                int use_min_score, const int* pos, const float* box_center, const float* box_scale, float* center,
                                float* scale, float* confidence, int* lost, int* keep_next, int* detected0, int* area0, int* claimed0) {
    const int b = blockIdx.x;
    const int p = pos[b];
    TrackBox r = {0.f, 0.f, 1.f, 0.f, 0};
    if (p >= 0) r = track_box_rule(kp_image, sm, cs, p, H, W, crop, margin, min_score, use_min_score);          // (p is uniform over the workgroup)
    if (threadIdx.x == 0) {
        const bool v = p >= 0;
        center[b * 2] = v ? r.cy : box_center[b * 2];
        center[b * 2 + 1] = v ? r.cx : box_center[b * 2 + 1];
        scale[b] = v ? r.scale : box_scale[b];
        confidence[b] = v ? r.conf : 0.f;
        lost[b] = v ? r.lost : 0;
        if (keep_next) keep_next[b] = (v && !r.lost) ? 1 : 0;
        if (detected0) detected0[b] = 0;
        if (area0) area0[b] = 0;
        if (claimed0) claimed0[b] = 0;
    }
}

// ---- detection on the lost frames only (option "track_partial_detect") ------------------------------------------------
// A detect step that only `lost` flags caused runs HandSegNet, the soft-max and the mask growth at batch m = the chunk's lost frames.
// idx [m] = those frames' indices in the chunk, ascending; pos [n] = a frame's dense index, -1 for one that keeps its tracked box.
//
// The two lists from the chunk's flags, on the device (the host knows m from its copy of the same flags): ONE workgroup walks the n flags
// 256 at a time -- an inclusive scan of the tile in LDS, the running count carried from tile to tile -- so any n works.
HP3D_KERNEL(256)
void track_partial_index_kernel(const int* lost, int n, int* idx, int* pos) {
    __shared__ int part[256];
    const int t = threadIdx.x;
    int base = 0;
    for (int b0 = 0; b0 < n; b0 += 256) {          // (uniform trip count: every lane reaches every barrier)
        const int b = b0 + t;
        const int flag = (b < n && lost[b] != 0) ? 1 : 0;
        part[t] = flag;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const int v = t >= d ? part[t - d] : 0;
            __syncthreads();
            part[t] += v;
            __syncthreads();
        }
        const int incl = part[t], tot = part[255];
        if (b < n) {
            const int p = base + incl - 1;
            pos[b] = flag ? p : -1;
            if (flag) idx[p] = b;
        }
        base += tot;
        __syncthreads();          // part is rewritten by the next tile
    }
}

// out[i] = frames[idx[i]], i < m; a frame is `words` units of VEC floats.  VEC = 4: 16-byte loads and stores (the frame's bytes a multiple
// of 16 and both bases 16-byte aligned, so every frame's base is); VEC = 1: 4 bytes.  The grid lies over (piece of a frame, frame);
// consecutive lanes take consecutive units.  src and dst must not overlap.
template <int VEC>
HP3D_KERNEL(256)
void frame_gather_kernel(const float* frames, const int* idx, int m, size_t words, float* out) {
    typedef typename std::conditional<VEC == 4, f32x4, float>::type vec_t;
    for (int i = blockIdx.y; i < m; i += gridDim.y) {
        const vec_t* sp = (const vec_t*)(frames + (size_t)idx[i] * words * VEC);
        vec_t* dp = (vec_t*)(out + (size_t)i * words * VEC);
        for (size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x; w < words; w += (size_t)gridDim.x * blockDim.x) dp[w] = sp[w];
    }
}

// preprocess_u8_kernel at equal sizes on the frames idx[i] only: out[i] = x / 255 - 0.5 of frame idx[i], float32 op by op (at equal sizes
// that kernel's result is its top-left tap); a frame is `words` units of VEC elements.  VEC = 4: one 4-byte load and one 16-byte store
// per lane (the frame's element count a multiple of 4, the source base 4-byte and the destination 16-byte aligned, so every frame's
// are); VEC = 1: element by element.
template <int VEC>
HP3D_KERNEL(256)
void preprocess_u8_idx_kernel(const unsigned char* img, const int* idx, int m, size_t words, float* out) {
    for (int i = blockIdx.y; i < m; i += gridDim.y) {
        const unsigned char* sp = img + (size_t)idx[i] * words * VEC;
        float* dp = out + (size_t)i * words * VEC;
        for (size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x; w < words; w += (size_t)gridDim.x * blockDim.x) {
            if (VEC == 4) {
                unsigned char v[4];
                __builtin_memcpy(v, __builtin_assume_aligned(sp + w * 4, 4), 4);
                f32x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = (float)v[e] / 255.0f - 0.5f;
                *(f32x4*)(dp + w * 4) = o;
            } else {
                dp[w] = (float)sp[w] / 255.0f - 0.5f;
            }
        }
    }
}

// track_select_kernel where HandSegNet ran on the lost frames only: det_center / det_scale are dense, image b's entry is pos[b].
HP3D_KERNEL(256)
void track_select_pos_kernel(const int* lost_prev, const int* pos, const float* det_center, const float* det_scale, int B,
                             float* box_center, float* box_scale, int* detected) {
    for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < B; b += gridDim.x * blockDim.x) {
        const int d = lost_prev[b] != 0 ? 1 : 0;
        if (d) {
            const int p = pos[b];
            box_center[b * 2] = det_center[p * 2]; box_center[b * 2 + 1] = det_center[p * 2 + 1];
            box_scale[b] = det_scale[p];
        }
        detected[b] = d;
    }
}

// ---- the multi-hand tracker's detection on the frames that lost a hand only (option "track_hands_partial_detect") ------
// A frame detects when one of its K slots is valid and lost, or when none is valid.  idx [m] = those frames' indices in the chunk,
// ascending; pos [n] = a frame's dense index, -1 for a frame whose slots all keep what they have.
//
// track_partial_index_kernel with the frame's flag reduced from its K valid | lost pairs first: ONE workgroup, n frames 256 at a time,
// the same inclusive scan in LDS and the same running count.
HP3D_KERNEL(256)
void track_hands_partial_index_kernel(const int* valid, const int* lost, int n, int K, int* idx, int* pos) {
    __shared__ int part[256];
    const int t = threadIdx.x;
    int base = 0;
    for (int b0 = 0; b0 < n; b0 += 256) {          // (uniform trip count: every lane reaches every barrier)
        const int b = b0 + t;
        int flag = 0;
        if (b < n) {
            bool any_valid = false, any_lost = false;
            for (int j = 0; j < K; ++j) {
                const bool v = valid[b * K + j] != 0;
                any_valid = any_valid || v;
                any_lost = any_lost || (v && lost[b * K + j] != 0);
            }
            flag = (any_lost || !any_valid) ? 1 : 0;
        }
        part[t] = flag;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const int v = t >= d ? part[t - d] : 0;
            __syncthreads();
            part[t] += v;
            __syncthreads();
        }
        const int incl = part[t], tot = part[255];
        if (b < n) {
            const int p = base + incl - 1;
            pos[b] = flag ? p : -1;
            if (flag) idx[p] = b;
        }
        base += tot;
        __syncthreads();          // part is rewritten by the next tile
    }
}

// keep / centre / scale of the K slots of the m frames idx[i] as dense [m, K] arrays for the claimed growth at batch m: latency only
HP3D_KERNEL(256)
void track_hands_slot_gather_kernel(const int* idx, int m, int K, const int* keep, const float* center, const float* scale, int* keep_d,
                                    float* center_d, float* scale_d) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < m * K; i += gridDim.x * blockDim.x) {
        const int s = idx[i / K] * K + i % K;
        keep_d[i] = keep[s];
        center_d[i * 2] = center[s * 2]; center_d[i * 2 + 1] = center[s * 2 + 1];
        scale_d[i] = scale[s];
    }
}

// track_hands_select_kernel where the claimed growth ran on the frames of idx only: the det_* arrays are dense [m, K], frame b's K entries
// at pos[b].  A slot of a frame with pos[b] < 0 keeps its box and its valid flag and gets detected = area = claimed = 0 (no object was
// looked for in that frame); the `claimed` counts of the others go back to their slots.
HP3D_KERNEL(256)
void track_hands_select_pos_kernel(const int* pos, int nb, int K, const int* keep, const float* det_center, const float* det_scale,
                                   const int* det_valid, const int* det_area, const int* det_claimed, float* box_center, float* box_scale,
                                   int* valid, int* detected, int* area, int* claimed) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nb * K; i += gridDim.x * blockDim.x) {
        const int p = pos[i / K];
        if (p < 0) {
            detected[i] = 0; area[i] = 0; claimed[i] = 0;
            continue;
        }
        const int d = p * K + i % K;
        claimed[i] = det_claimed[d];
        if (keep[i]) {
            valid[i] = 1; detected[i] = 0; area[i] = 0;
        } else {
            const int v = det_valid[d] != 0 ? 1 : 0;
            box_center[i * 2] = det_center[d * 2]; box_center[i * 2 + 1] = det_center[d * 2 + 1];
            box_scale[i] = det_scale[d];
            valid[i] = v; detected[i] = v; area[i] = v ? det_area[d] : 0;
        }
    }
}

inline int grid_for(long total, int block = 256, int cap = 256 * 16) {
    long g = (total + block - 1) / block;
    if (g < 1) g = 1;
    return (int)(g > cap ? cap : g);
}

}  // namespace

// ---- launchers ---------------------------------------------------------------------------
void conv_naive_launch(const float* x, int B, int H, int W, int Cin, int in_cs, const float* w, const float* bias,
                       int k, int stride, int Cout, int act, float* out, int out_cs, int Ho, int Wo, int pad_t,
                       int pad_l, hipStream_t s) {
    HP3D_LAUNCH(conv_naive_kernel, dim3(grid_for((long)B * Ho * Wo * Cout)), dim3(256), 0, s, x, B, H, W, Cin, in_cs,
                w, bias, k, stride, Cout, act, out, out_cs, Ho, Wo, pad_t, pad_l);
}
void conv_splitk_reduce_launch(const float* partial, int ksplit, long npix, int Cout, const float* bias, int act,
                               float* out, int out_cs, int cout_store, hipStream_t s) {
    const bool v4 = !((Cout | out_cs | cout_store) & 3) && !(((uintptr_t)partial | (uintptr_t)bias | (uintptr_t)out) & 15);
    if (v4) HP3D_LAUNCH(conv_splitk_reduce_kernel<4>, dim3(grid_for(npix * (cout_store / 4))), dim3(256), 0, s, partial, ksplit, npix,
                        Cout, bias, act, out, out_cs, cout_store);
    else HP3D_LAUNCH(conv_splitk_reduce_kernel<1>, dim3(grid_for(npix * cout_store)), dim3(256), 0, s, partial, ksplit, npix,
                     Cout, bias, act, out, out_cs, cout_store);
}
void conv_splitk_reduce_pool_launch(const float* partial, int ksplit, int B, int H, int W, int Cout, const float* bias, int act,
                                    float* out, int out_cs, int cout_store, hipStream_t s) {
    HP3D_LAUNCH(conv_splitk_reduce_pool_kernel, dim3(grid_for((long)B * (H / 2) * (W / 2) * cout_store)), dim3(256), 0, s, partial, ksplit,
                B, H, W, Cout, bias, act, out, out_cs, cout_store);
}
void maxpool2_launch(const float* x, int B, int H, int W, int C, int in_cs, float* out, hipStream_t s) {
    HP3D_LAUNCH(maxpool2_kernel, dim3(grid_for((long)B * (H / 2) * (W / 2) * C)), dim3(256), 0, s, x, B, H, W, C,
                in_cs, out);
}
void avgpool8_launch(const float* x, int B, int H, int W, int C, float* out, int out_cs, hipStream_t s) {
    HP3D_LAUNCH(avgpool8_kernel, dim3(grid_for((long)B * (H / 8) * (W / 8) * C)), dim3(256), 0, s, x, B, H, W, C,
                out, out_cs);
}
void resize_bilinear_launch(const float* x, int B, int H, int W, int C, int in_cs, int oh, int ow, float* out,
                            hipStream_t s) {
    const long total = (long)B * oh * ow * C;
    const size_t row_lds = ((size_t)2 * W * C + (size_t)3 * ow) * 4;
    // (exact px = i / C from the float reciprocal needs i < 2^20 or so: W x C and ow x C are far below)
    if ((ow * C) % 4 == 0 && ((uintptr_t)out & 15) == 0 && row_lds <= 60 * 1024 && (long)ow * C < (1L << 20) && (long)W * C < (1L << 20) && B <= 65535 &&
        oh >= 4 * H) {
        HP3D_LAUNCH(resize_bilinear_rows_kernel, dim3(oh, B), dim3(256), row_lds, s, x, H, W, C, in_cs, oh, ow, out, 1.0f / (float)C);
        return;
    }
    if (total < (1L << 31)) {
        auto k32 = resize_bilinear_kernel<unsigned>;
        HP3D_LAUNCH(k32, dim3(grid_for(total, 256, 256 * 32)), dim3(256), 0, s, x, B, H, W, C, in_cs, oh, ow, out);
    } else {
        auto k64 = resize_bilinear_kernel<unsigned long>;
        HP3D_LAUNCH(k64, dim3(grid_for(total, 256, 256 * 32)), dim3(256), 0, s, x, B, H, W, C, in_cs, oh, ow, out);
    }
}
void preprocess_u8_launch(const unsigned char* img, int B, int H, int W, int oh, int ow, float* out, hipStream_t s) {
    HP3D_LAUNCH(preprocess_u8_kernel, dim3(grid_for((long)B * oh * ow * 3)), dim3(256), 0, s, img, B, H, W, oh, ow, out);
}
void crop_and_resize_launch(const float* img, int B, int H, int W, int C, const float* center, const float* scale,
                            int crop, float* out, hipStream_t s, int boxes_per_image) {
    HP3D_LAUNCH(crop_and_resize_kernel, dim3(grid_for((long)B * crop * crop)), dim3(256), 0, s, img, B, H, W, C,
                center, scale, crop, out, boxes_per_image);
}
// Streams `n` floats through the caches and keeps nothing (the store below never executes for finite data): what it leaves behind is
// the buffer resident in the memory-side cache for the gather loads of the kernel that follows (option "first_touch").
HP3D_KERNEL(256)
void touch_kernel(const float* p, long n4, float* sink) {
    const f32x4* q = (const f32x4*)p;
    float acc = 0.f;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const f32x4 v = q[i];
        acc += v[0] + v[1] + v[2] + v[3];
    }
    if (acc == 1.2345e-38f) *sink = acc;
}
void touch_launch(const float* p, size_t nfloats, float* sink, hipStream_t s) {
    const long n4 = (long)(nfloats / 4);
    if (n4 < 1 || ((uintptr_t)p & 15)) return;
    HP3D_LAUNCH(touch_kernel, dim3(grid_for(n4, 256, 256 * 8)), dim3(256), 0, s, p, n4, sink);
}
void copy_channels_launch(const float* in, int npix, int C, int in_cs, float* out, int out_cs, hipStream_t s) {
    HP3D_LAUNCH(copy_channels_kernel, dim3(grid_for((long)npix * C)), dim3(256), 0, s, in, (long)npix, C, in_cs, out,
                out_cs);
}
void cvt_channels_f16_launch(const float* in, int npix, int C, int in_cs, hp3d_f16* out, int out_cs, hipStream_t s) {
    HP3D_LAUNCH(cvt_channels_f16_kernel, dim3(grid_for((long)npix * C)), dim3(256), 0, s, in, (long)npix, C, in_cs, out,
                out_cs);
}
void pad_channels_launch(const float* in, int npix, int C, float* out, int out_cs, hipStream_t s) {
    HP3D_LAUNCH(pad_channels_kernel, dim3(grid_for((long)npix * out_cs)), dim3(256), 0, s, in, (long)npix, C, out,
                out_cs);
}
void seg_upsample_softmax_launch(const float* small, int B, int hs, int ws, int cs, int H, int W,
                                 float* scoremap_large, const MaskBuffers& mb, hipStream_t s) {
    (void)hipMemsetAsync(mb.argmax_key, 0, sizeof(unsigned long long) * B, s);
    const int gx = grid_for((long)H * W, 256, 64);
    HP3D_LAUNCH(seg_upsample_softmax_kernel, dim3(gx, B), dim3(256), 0, s, small, B, hs, ws, cs, H, W, scoremap_large,
                mb.det, mb.fg, mb.argmax_key);
}
void seg_softmax_launch(const float* scoremap_large, int B, int H, int W, const MaskBuffers& mb, hipStream_t s) {
    (void)hipMemsetAsync(mb.argmax_key, 0, sizeof(unsigned long long) * B, s);
    const int gx = grid_for((long)H * W, 256, 64);
    HP3D_LAUNCH(seg_softmax_kernel, dim3(gx, B), dim3(256), 0, s, scoremap_large, B, H, W, mb.det, mb.fg,
                mb.argmax_key);
}
// three bitmaps of H rows x (ceil(W / 32) + 1 guard) words, + the two end guards of the growing one
size_t mask_grow_lds_bytes(int H, int W) { return ((size_t)3 * H * ((W + 31) / 32 + 1) + 2) * sizeof(unsigned); }
bool mask_grow_lds_fits(int H, int W) { return mask_grow_lds_bytes(H, W) <= 160 * 1024 - 1024; }
size_t mask_grow_global_words(int H, int W) { return (size_t)3 * H * ((W + 31) / 32 + 1) + 2; }
void mask_grow_global_launch(const MaskBuffers& mb, int B, int H, int W, int empty_fltmax, unsigned* scratch, float* mask_out,
                             float* center, float* crop_size, float* scale, int* seed, hipStream_t s) {
    const long nword = (long)H * ((W + 31) / 32 + 1);
    HP3D_LAUNCH(mask_pack_kernel, dim3(grid_for(nword, 256, 64), B), dim3(256), 0, s, (const unsigned char*)mb.det,
                (const unsigned long long*)mb.argmax_key, H, W, scratch);
    HP3D_LAUNCH(mask_grow_global_kernel, dim3(B), dim3(1024), 0, s, (const unsigned long long*)mb.argmax_key, H, W, empty_fltmax,
                scratch, mask_out, center, crop_size, scale, seed);
}
void mask_grow_launch(const MaskBuffers& mb, int B, int H, int W, int empty_fltmax, float* mask_out, float* center,
                      float* crop_size, float* scale, int* seed, hipStream_t s) {
    const size_t smem = mask_grow_lds_bytes(H, W);
    static bool attr_done[64] = {};
    if (hp3d_first_use_on_device(attr_done))
        (void)hipFuncSetAttribute((const void*)mask_grow_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 64);
    HP3D_LAUNCH(mask_grow_kernel, dim3(B), dim3(1024), smem, s, (const unsigned char*)mb.det,
                (const unsigned long long*)mb.argmax_key, H, W, empty_fltmax, mask_out, center, crop_size, scale, seed);
}
// B images, K slots each: outputs at index b * K + j.  scratch: null = the LDS kernel, else B x mask_grow_global_words(H, W) words
void mask_grow_multi_launch(const MaskBuffers& mb, int B, int H, int W, int K, int min_area, int empty_fltmax, unsigned* scratch,
                            float* mask_out, float* center, float* crop_size, float* scale, int* seed, int* valid, int* area, hipStream_t s,
                            const MaskKeep& mk) {
    if (scratch) {
        const long nword = (long)H * ((W + 31) / 32 + 1);
        HP3D_LAUNCH(mask_pack_kernel, dim3(grid_for(nword, 256, 64), B), dim3(256), 0, s, (const unsigned char*)mb.det,
                    (const unsigned long long*)mb.argmax_key, H, W, scratch);
        HP3D_LAUNCH(mask_grow_multi_global_kernel, dim3(B), dim3(1024), 0, s, (const float*)mb.fg, (const unsigned long long*)mb.argmax_key,
                    H, W, K, min_area, empty_fltmax, scratch, mask_out, center, crop_size, scale, seed, valid, area, mk.keep, mk.center, mk.scale,
                    mk.claimed);
        return;
    }
    const size_t smem = mask_grow_lds_bytes(H, W);
    static bool attr_done[64] = {};
    if (hp3d_first_use_on_device(attr_done))
        // (dynamic + static LDS must stay within 160 KB: the kernel's own statics -- flags, box, the arg-max's per-wave keys -- take under
        //  256 bytes, and mask_grow_lds_fits admits maps of at most 160 KB - 1 KB)
        (void)hipFuncSetAttribute((const void*)mask_grow_multi_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 1024);
    HP3D_LAUNCH(mask_grow_multi_kernel, dim3(B), dim3(1024), smem, s, (const unsigned char*)mb.det, (const float*)mb.fg,
                (const unsigned long long*)mb.argmax_key, H, W, K, min_area, empty_fltmax, mask_out, center, crop_size, scale, seed, valid, area,
                mk.keep, mk.center, mk.scale, mk.claimed);
}
size_t fc_scratch_floats(int B, int Cin, int Cout) { return (size_t)((Cin + FC_KCH - 1) / FC_KCH) * B * Cout; }
void fc_launch(const float* x, int B, int Cin, int x_stride, const float* w, const float* bias, int Cout, int act,
               float* out, int out_stride, float* scratch, hipStream_t s, const float* x2, int F1) {
    const int ns = (Cin + FC_KCH - 1) / FC_KCH;
    HP3D_LAUNCH(fc_partial_kernel, dim3((Cout + 63) / 64, ns, (B + FC_BT - 1) / FC_BT), dim3(256), 0, s, x, B, Cin,
                x_stride, x2, x2 ? F1 : Cin, w, Cout, scratch, 0, 0);
    HP3D_LAUNCH(fc_reduce_kernel, dim3(grid_for((long)B * Cout)), dim3(256), 0, s, (const float*)scratch, ns, B, Cout,
                bias, act, out, out_stride);
}
// the K slices only (the reduction happens in the consumer: fc_tail_launch); returns the slice count
int fc_partial_launch(const float* x, int B, int Cin, int x_stride, const float* w, int Cout, float* scratch, hipStream_t s, const float* x2, int F1) {
    const int ns = (Cin + FC_KCH - 1) / FC_KCH;
    HP3D_LAUNCH(fc_partial_kernel, dim3((Cout + 63) / 64, ns, (B + FC_BT - 1) / FC_BT), dim3(256), 0, s, x, B, Cin,
                x_stride, x2, x2 ? F1 : Cin, w, Cout, scratch, 0, 0);
    return ns;
}
int fc_tail_eligible(int C0, int C1, int C2) { return C0 <= FCT_MAXC && C2 >= 1 && C1 <= FCT_MAXC && C1 >= 4 && C1 % 4 == 0 && 256 % (C1 / 4) == 0 && (256 / (C1 / 4)) <= 8; }
void fc_tail_launch(const float* part0, int ns0, int B, int C0, const float* bias0, int act0, const float* w1, const float* b1, int C1, int act1,
                    const float* w2, const float* b2, int C2, int act2, float* out, int out_stride, hipStream_t s) {
    HP3D_LAUNCH(fc_tail_kernel, dim3((B + FCT_G - 1) / FCT_G), dim3(256), 0, s, part0, ns0, B, C0, bias0, act0, w1, b1, C1, act1, w2, b2, C2, act2, out, out_stride);
}
// a 3x3 / stride-2 / SAME convolution of an [n,S,S,C] map (S even) as split-K GEMM over its S/2 x S/2 x n output pixels; w = the HWIO filter;
// scratch: fc_scratch_floats(n * (S/2)^2, 9 C, Cout)
void conv_s2_gemm_launch(const float* x, int n, int S, int C, const float* w_hwio, const float* bias, int Cout, int act, float* out, float* scratch, hipStream_t s) {
    const int rows = n * (S / 2) * (S / 2), K = 9 * C, ns = (K + FC_KCH - 1) / FC_KCH;
    HP3D_LAUNCH(fc_partial_kernel, dim3((Cout + 63) / 64, ns, (rows + FC_BT - 1) / FC_BT), dim3(256), 0, s, x, rows, K, 0, (const float*)nullptr, K, w_hwio, Cout, scratch, S, C);
    HP3D_LAUNCH(fc_reduce_kernel, dim3(grid_for((long)rows * Cout)), dim3(256), 0, s, (const float*)scratch, ns, rows, Cout, bias, act, out, Cout);
}
void lift_epilogue_launch(const float* u, const float* coord_can, const float* hand_side, int B, float* rot,
                          float* coord_rel, int do_flip_rot, hipStream_t s) {
    HP3D_LAUNCH(lift_epilogue_kernel, dim3((B + 63) / 64), dim3(64), 0, s, u, coord_can, hand_side, B, rot, coord_rel,
                do_flip_rot);
}
void bone_rel_inv_launch(const float* rel, int B, float* xyz, hipStream_t s) {
    HP3D_LAUNCH(bone_rel_inv_kernel, dim3((B + 63) / 64), dim3(64), 0, s, rel, B, xyz);
}
void kp_detect_launch(const float* sm, int B, int h, int w, int C, int cs, int oh, int ow, const float* scale,
                      const float* center, int* kp_crop, double* kp_image, hipStream_t s) {
    HP3D_LAUNCH(kp_detect_kernel, dim3(C, B), dim3(256), 0, s, sm, h, w, C, cs, oh, ow, scale, center, kp_crop, kp_image);
}
void crop_and_resize_u8_launch(const unsigned char* img, int B, int H, int W, const float* center, const float* scale, int crop,
                               float* out, hipStream_t s, int boxes_per_image) {
    HP3D_LAUNCH(crop_and_resize_u8_kernel, dim3(grid_for((long)B * crop * crop)), dim3(256), 0, s, img, B, H, W, center, scale,
                crop, out, boxes_per_image);
}
void track_box_launch(const double* kp_image, const float* sm, int cs, int B, int H, int W, int crop, float margin, float min_score,
                      int use_min_score, float* center, float* scale, float* confidence, int* lost, int* detected0, hipStream_t s) {
    HP3D_LAUNCH(track_box_kernel, dim3(B), dim3(256), 0, s, kp_image, sm, cs, H, W, crop, margin, min_score, use_min_score, center,
                scale, confidence, lost, detected0);
}
void track_select_launch(const int* lost_prev, const float* det_center, const float* det_scale, int B, int force_all,
                         float* box_center, float* box_scale, int* detected, hipStream_t s) {
    HP3D_LAUNCH(track_select_kernel, dim3(grid_for(B)), dim3(256), 0, s, lost_prev, det_center, det_scale, B, force_all, box_center,
                box_scale, detected);
}
void track_hands_box_launch(const double* kp_image, const float* sm, int cs, int n, int H, int W, int crop, float margin, float min_score,
                            int use_min_score, const int* valid, const float* box_center, const float* box_scale, float* center, float* scale,
                            float* confidence, int* lost, int* keep_next, int* detected0, int* area0, int* claimed0, hipStream_t s) {
    HP3D_LAUNCH(track_hands_box_kernel, dim3(n), dim3(256), 0, s, kp_image, sm, cs, H, W, crop, margin, min_score, use_min_score, valid,
                box_center, box_scale, center, scale, confidence, lost, keep_next, detected0, area0, claimed0);
}
void crop_and_resize_idx_launch(const float* img, int m, int H, int W, int C, const float* center, const float* scale, const int* idx, int K,
                                int crop, float* out, hipStream_t s) {
    HP3D_LAUNCH(crop_and_resize_idx_kernel, dim3(grid_for((long)m * crop * crop)), dim3(256), 0, s, img, m, H, W, C, center, scale, idx, K,
                crop, out);
}
void crop_and_resize_idx_u8_launch(const unsigned char* img, int m, int H, int W, const float* center, const float* scale, const int* idx,
                                   int K, int crop, float* out, hipStream_t s) {
    HP3D_LAUNCH(crop_and_resize_idx_u8_kernel, dim3(grid_for((long)m * crop * crop)), dim3(256), 0, s, img, m, H, W, center, scale, idx, K,
                crop, out);
}
void slot_gather_launch(const int* idx, int m, const float* hand_side, const float* center, const float* scale, float* hand_side_d,
                        float* center_d, float* scale_d, hipStream_t s) {
    HP3D_LAUNCH(slot_gather_kernel, dim3(grid_for(m)), dim3(256), 0, s, idx, m, hand_side, center, scale, hand_side_d, center_d, scale_d);
}
void slot_scatter_launch(ScatterPlan plan, const int* pos, int ns, hipStream_t s) {
    if (plan.n < 1 || ns < 1) return;
    unsigned segs = 0;
    for (int i = 0; i < plan.n; ++i) {
        ScatterArray& a = plan.a[i];
        a.seg0 = segs;
        a.vec = !(a.words & 3) && !(((uintptr_t)a.src | (uintptr_t)a.dst) & 15);          // (conv_splitk_reduce_launch's choice)
        segs += (a.words + SCATTER_SEG_WORDS - 1) / SCATTER_SEG_WORDS;
    }
    HP3D_LAUNCH(slot_scatter_kernel, dim3(segs, std::min(ns, 65535)), dim3(256), 0, s, plan, pos, ns);
}
void track_hands_box_pos_launch(const double* kp_image, const float* sm, int cs, int n, int H, int W, int crop, float margin, float min_score,
                                int use_min_score, const int* pos, const float* box_center, const float* box_scale, float* center,
                                float* scale, float* confidence, int* lost, int* keep_next, int* detected0, int* area0, int* claimed0,
                                hipStream_t s) {
    HP3D_LAUNCH(track_hands_box_pos_kernel, dim3(n), dim3(256), 0, s, kp_image, sm, cs, H, W, crop, margin, min_score, use_min_score, pos,
                box_center, box_scale, center, scale, confidence, lost, keep_next, detected0, area0, claimed0);
}
void track_hands_select_launch(const int* keep, const float* det_center, const float* det_scale, const int* det_valid, const int* det_area,
                               int n, float* box_center, float* box_scale, int* valid, int* detected, int* area, hipStream_t s) {
    HP3D_LAUNCH(track_hands_select_kernel, dim3(grid_for(n)), dim3(256), 0, s, keep, det_center, det_scale, det_valid, det_area, n,
                box_center, box_scale, valid, detected, area);
}
void track_partial_index_launch(const int* lost, int n, int* idx, int* pos, hipStream_t s) {
    HP3D_LAUNCH(track_partial_index_kernel, dim3(1), dim3(256), 0, s, lost, n, idx, pos);
}
void frame_gather_launch(const float* frames, const int* idx, int m, size_t frame_floats, float* out, hipStream_t s) {
    if (m < 1 || frame_floats < 1) return;
    const bool vec = !(frame_floats & 3) && !(((uintptr_t)frames | (uintptr_t)out) & 15);
    const size_t words = vec ? frame_floats / 4 : frame_floats;
    const dim3 grid(grid_for((long)words, 256, 1024), std::min(m, 65535)), block(256);
    if (vec) HP3D_LAUNCH(frame_gather_kernel<4>, grid, block, 0, s, frames, idx, m, words, out);
    else HP3D_LAUNCH(frame_gather_kernel<1>, grid, block, 0, s, frames, idx, m, words, out);
}
void preprocess_u8_idx_launch(const unsigned char* img, const int* idx, int m, int H, int W, float* out, hipStream_t s) {
    if (m < 1) return;
    const size_t n = (size_t)H * W * 3;
    const bool vec = !(n & 3) && !((uintptr_t)img & 3) && !((uintptr_t)out & 15);
    const size_t words = vec ? n / 4 : n;
    const dim3 grid(grid_for((long)words, 256, 1024), std::min(m, 65535)), block(256);
    if (vec) HP3D_LAUNCH(preprocess_u8_idx_kernel<4>, grid, block, 0, s, img, idx, m, words, out);
    else HP3D_LAUNCH(preprocess_u8_idx_kernel<1>, grid, block, 0, s, img, idx, m, words, out);
}
void track_select_pos_launch(const int* lost_prev, const int* pos, const float* det_center, const float* det_scale, int B,
                             float* box_center, float* box_scale, int* detected, hipStream_t s) {
    HP3D_LAUNCH(track_select_pos_kernel, dim3(grid_for(B)), dim3(256), 0, s, lost_prev, pos, det_center, det_scale, B, box_center,
                box_scale, detected);
}
void track_hands_partial_index_launch(const int* valid, const int* lost, int n, int K, int* idx, int* pos, hipStream_t s) {
    HP3D_LAUNCH(track_hands_partial_index_kernel, dim3(1), dim3(256), 0, s, valid, lost, n, K, idx, pos);
}
void track_hands_slot_gather_launch(const int* idx, int m, int K, const int* keep, const float* center, const float* scale, int* keep_d,
                                    float* center_d, float* scale_d, hipStream_t s) {
    if (m < 1) return;
    HP3D_LAUNCH(track_hands_slot_gather_kernel, dim3(grid_for((long)m * K)), dim3(256), 0, s, idx, m, K, keep, center, scale, keep_d,
                center_d, scale_d);
}
void track_hands_select_pos_launch(const int* pos, int nb, int K, const int* keep, const float* det_center, const float* det_scale,
                                   const int* det_valid, const int* det_area, const int* det_claimed, float* box_center, float* box_scale,
                                   int* valid, int* detected, int* area, int* claimed, hipStream_t s) {
    HP3D_LAUNCH(track_hands_select_pos_kernel, dim3(grid_for((long)nb * K)), dim3(256), 0, s, pos, nb, K, keep, det_center, det_scale,
                det_valid, det_area, det_claimed, box_center, box_scale, valid, detected, area, claimed);
}
// T = float | unsigned char; the wide form where f is 2, 4 or 8 and every window row starts on the load's alignment
template <typename T>
static int downscale_wide(const T* img, int W, int f) {
    const int rowb = f * 3 * (int)sizeof(T);
    const int align = rowb % 16 == 0 ? 16 : rowb % 8 == 0 ? 8 : rowb % 4 == 0 ? 4 : rowb % 2 == 0 ? 2 : 1;
    return ((uintptr_t)img % align == 0 && ((size_t)W * 3 * sizeof(T)) % align == 0) ? 1 : 0;
}
// ... a packed surface: the base, the pitch and the stride (0 where one frame is reached) on the alignment of the load
// that downscale_px_body takes a window row of f pixels with
static int downscale_wide(const PxSrc& P, int, int f) {
    const int rowb = f * P.pixel_bytes;
    const int align = rowb % 16 == 0 ? 16 : rowb % 8 == 0 ? 8 : rowb % 4 == 0 ? 4 : rowb % 2 == 0 ? 2 : 1;
    return ((uintptr_t)P.px % align == 0 && P.pitch % align == 0 && P.frame_stride % align == 0) ? 1 : 0;
}
// One dispatcher for both forms: `lead...` = (B) for the kernels over the whole batch, (idx, m) for the indexed ones -- where the same
// test holds: a frame is H row pitches long, so every selected frame's base is aligned as the first one's.
// (Src = const T* or a PxSrc: whatever downscale_wide takes and the kernels take first)
template <typename Src, class K0, class K2, class K4, class K8, class... Lead>
static void downscale_dispatch(K0 k0, K2 k2, K4 k4, K8 k8, const Src img, int frames, int H, int W, int f, float* out, hipStream_t s,
                               Lead... lead) {
    if (frames < 1) return;
    const int Hd = (H + f - 1) / f, Wd = (W + f - 1) / f;
    const int wide = downscale_wide(img, W, f);
    const dim3 grid(grid_for((long)frames * Hd * Wd)), block(256);
    if (f == 2) HP3D_LAUNCH(k2, grid, block, 0, s, img, lead..., H, W, f, Hd, Wd, wide, out);
    else if (f == 4) HP3D_LAUNCH(k4, grid, block, 0, s, img, lead..., H, W, f, Hd, Wd, wide, out);
    else if (f == 8) HP3D_LAUNCH(k8, grid, block, 0, s, img, lead..., H, W, f, Hd, Wd, wide, out);
    else HP3D_LAUNCH(k0, grid, block, 0, s, img, lead..., H, W, f, Hd, Wd, 0, out);
}
void downscale_idx_launch(const float* img, const int* idx, int m, int H, int W, int f, float* out, hipStream_t s) {
    downscale_dispatch(downscale_idx_kernel<0>, downscale_idx_kernel<2>, downscale_idx_kernel<4>, downscale_idx_kernel<8>, img, m, H, W, f,
                       out, s, idx, m);
}
void downscale_u8_idx_launch(const unsigned char* img, const int* idx, int m, int H, int W, int f, float* out, hipStream_t s) {
    downscale_dispatch(downscale_u8_idx_kernel<0>, downscale_u8_idx_kernel<2>, downscale_u8_idx_kernel<4>, downscale_u8_idx_kernel<8>, img,
                       m, H, W, f, out, s, idx, m);
}
void downscale_launch(const float* img, int B, int H, int W, int f, float* out, hipStream_t s) {
    downscale_dispatch(downscale_kernel<0>, downscale_kernel<2>, downscale_kernel<4>, downscale_kernel<8>, img, B, H, W, f, out, s, B);
}
void downscale_u8_launch(const unsigned char* img, int B, int H, int W, int f, float* out, hipStream_t s) {
    downscale_dispatch(downscale_u8_kernel<0>, downscale_u8_kernel<2>, downscale_u8_kernel<4>, downscale_u8_kernel<8>, img, B, H, W, f, out, s, B);
}
// ---- NV12 frames ----
int nv12_matrix_index(const char* name) {
    static const char* names[] = {"bt709", "bt601", "bt709_full", "bt601_full"};
    for (int i = 0; i < 4; ++i)
        if (!strcmp(name, names[i])) return i;
    return -1;
}
Nv12Src nv12_src(const unsigned char* y, const unsigned char* uv, int pitch, size_t frame_stride, int matrix) {
    // {ky, yoff, R's cv, G's cu, G's cv, B's cu}: the rounded coefficients ARE the definition (include/hp3d.h)
    static const int coef[4][6] = {{298, 16, 459, -55, -136, 541}, {298, 16, 409, -100, -208, 516}, {256, 0, 403, -48, -120, 475},
                                   {256, 0, 359, -88, -183, 454}};
    const int* c = coef[matrix >= 0 && matrix < 4 ? matrix : 0];
    return Nv12Src{y, uv, pitch, frame_stride, c[0], c[1], c[2], c[3], c[4], c[5]};
}
void nv12_to_rgb_launch(const Nv12Src& src, int B, int H, int W, unsigned char* out, hipStream_t s) {
    HP3D_LAUNCH(nv12_to_rgb_kernel, dim3(grid_for((long)B * H * (W / 2))), dim3(256), 0, s, src, B, H, W, out);
}
void crop_and_resize_nv12_launch(const Nv12Src& src, int n, int H, int W, const float* center, const float* scale, const int* idx, int K,
                                 int crop, float* out, hipStream_t s) {
    if (n < 1) return;
    const dim3 grid(grid_for((long)n * crop * crop)), block(256);
    if (idx) HP3D_LAUNCH(crop_and_resize_idx_nv12_kernel, grid, block, 0, s, src, n, H, W, center, scale, idx, K, crop, out);
    else HP3D_LAUNCH(crop_and_resize_nv12_kernel, grid, block, 0, s, src, n, H, W, center, scale, crop, out, K);
}
void downscale_nv12_launch(const Nv12Src& src, const int* idx, int frames, int H, int W, int f, float* out, hipStream_t s) {
    if (frames < 1) return;
    if (f == 1) {
        const dim3 grid(grid_for((long)frames * H * (W / 2))), block(256);
        if (idx) HP3D_LAUNCH(preprocess_nv12_kernel<true>, grid, block, 0, s, src, idx, frames, H, W, out);
        else HP3D_LAUNCH(preprocess_nv12_kernel<false>, grid, block, 0, s, src, idx, frames, H, W, out);
        return;
    }
    const int Hd = (H + f - 1) / f, Wd = (W + f - 1) / f;
    // wide: every window row of both planes starts on an f-byte boundary (the stride only counts where a second frame is reached).
    // It is decided on the device addresses, so nothing a caller sees says which path ran, and both give the same bits.  A tight
    // upload of one surface (hp3d_downscale_nv12) puts the chroma plane at y + stride (B - 1) + pitch (H - 1) + W: an unused row
    // between the planes or an odd span sends such a call down the element path whatever the pitch is.
    const bool one = frames == 1 && !idx;
    const int wide = (f == 2 || f == 4 || f == 8) && (uintptr_t)src.y % f == 0 && (uintptr_t)src.uv % f == 0 && src.pitch % f == 0 &&
                     (one || src.frame_stride % f == 0) ? 1 : 0;
    const dim3 grid(grid_for((long)frames * Hd * Wd)), block(256);
    if (idx) {
        if (f == 2) HP3D_LAUNCH(downscale_nv12_idx_kernel<2>, grid, block, 0, s, src, idx, frames, H, W, f, Hd, Wd, wide, out);
        else if (f == 4) HP3D_LAUNCH(downscale_nv12_idx_kernel<4>, grid, block, 0, s, src, idx, frames, H, W, f, Hd, Wd, wide, out);
        else if (f == 8) HP3D_LAUNCH(downscale_nv12_idx_kernel<8>, grid, block, 0, s, src, idx, frames, H, W, f, Hd, Wd, wide, out);
        else HP3D_LAUNCH(downscale_nv12_idx_kernel<0>, grid, block, 0, s, src, idx, frames, H, W, f, Hd, Wd, 0, out);
    } else {
        if (f == 2) HP3D_LAUNCH(downscale_nv12_kernel<2>, grid, block, 0, s, src, frames, H, W, f, Hd, Wd, wide, out);
        else if (f == 4) HP3D_LAUNCH(downscale_nv12_kernel<4>, grid, block, 0, s, src, frames, H, W, f, Hd, Wd, wide, out);
        else if (f == 8) HP3D_LAUNCH(downscale_nv12_kernel<8>, grid, block, 0, s, src, frames, H, W, f, Hd, Wd, wide, out);
        else HP3D_LAUNCH(downscale_nv12_kernel<0>, grid, block, 0, s, src, frames, H, W, f, Hd, Wd, 0, out);
    }
}
// ---- packed 8-bit frames ----
int px_pixel_bytes(int format) { return format < 0 || format > 5 ? 0 : format < 2 ? 3 : 4; }
PxSrc px_src(const unsigned char* px, int pitch, size_t frame_stride, int format) {
    // the byte offsets of R, G, B: HP3D_PX_RGB, BGR, RGBA, BGRA, ARGB, ABGR (include/hp3d.h)
    static const int off[6][3] = {{0, 1, 2}, {2, 1, 0}, {0, 1, 2}, {2, 1, 0}, {1, 2, 3}, {3, 2, 1}};
    const int* o = off[format >= 0 && format < 6 ? format : 0];
    const int pb = px_pixel_bytes(format);
    const int wide = (pb == 4 && (uintptr_t)px % 4 == 0 && pitch % 4 == 0 && frame_stride % 4 == 0) ? 1 : 0;
    return PxSrc{px, pitch, frame_stride, pb, o[0], o[1], o[2], wide};
}
void px_to_rgb_launch(const PxSrc& src, int B, int H, int W, unsigned char* out, hipStream_t s) {
    HP3D_LAUNCH(px_to_rgb_kernel, dim3(grid_for((long)B * H * W)), dim3(256), 0, s, src, B, H, W, out);
}
void crop_and_resize_px_launch(const PxSrc& src, int n, int H, int W, const float* center, const float* scale, const int* idx, int K,
                               int crop, float* out, hipStream_t s) {
    if (n < 1) return;
    const dim3 grid(grid_for((long)n * crop * crop)), block(256);
    if (idx) HP3D_LAUNCH(crop_and_resize_idx_px_kernel, grid, block, 0, s, src, n, H, W, center, scale, idx, K, crop, out);
    else HP3D_LAUNCH(crop_and_resize_px_kernel, grid, block, 0, s, src, n, H, W, center, scale, crop, out, K);
}
void downscale_px_launch(const PxSrc& src, const int* idx, int frames, int H, int W, int f, float* out, hipStream_t s) {
    if (frames < 1) return;
    if (f == 1) {
        const dim3 grid(grid_for((long)frames * H * W)), block(256);
        if (idx) HP3D_LAUNCH(preprocess_px_kernel<true>, grid, block, 0, s, src, idx, frames, H, W, out);
        else HP3D_LAUNCH(preprocess_px_kernel<false>, grid, block, 0, s, src, idx, frames, H, W, out);
        return;
    }
    if (idx)
        downscale_dispatch(downscale_px_idx_kernel<0>, downscale_px_idx_kernel<2>, downscale_px_idx_kernel<4>, downscale_px_idx_kernel<8>, src,
                           frames, H, W, f, out, s, idx, frames);
    else
        downscale_dispatch(downscale_px_kernel<0>, downscale_px_kernel<2>, downscale_px_kernel<4>, downscale_px_kernel<8>, src, frames, H, W,
                           f, out, s, frames);
}
// ---- a batch of separate surfaces ----
// One record from one surface's OWN address and pitch (a device address: the facts are about what the kernels load).  wide: PxSrc::wide;
// dwide bit f (f = 2, 4, 8): the wide window loads of that f -- downscale_wide's test for a packed surface, both planes and the pitch on
// an f-byte grid for an NV12 one, each as for a batch of one frame.
SurfRec surf_rec(const unsigned char* data, const unsigned char* chroma, int pitch, int format) {
    SurfRec R{};
    R.data = data; R.chroma = chroma; R.pitch = pitch;
    if (format == HP3D_SURF_FORMAT_NV12) {
        R.nv12 = 1;
        for (int f = 2; f <= 8; f *= 2)
            if ((uintptr_t)data % f == 0 && (uintptr_t)chroma % f == 0 && pitch % f == 0) R.dwide |= 1 << f;
        return R;
    }
    const PxSrc P = px_src(data, pitch, 0, format);
    R.chroma = nullptr;
    R.pixel_bytes = P.pixel_bytes; R.ro = P.ro; R.go = P.go; R.bo = P.bo; R.wide = P.wide;
    for (int f = 2; f <= 8; f *= 2)
        if (downscale_wide(P, 0, f)) R.dwide |= 1 << f;
    return R;
}
SurfSrc surf_src(const SurfRec* d_rec, int matrix) {
    const Nv12Src c = nv12_src(nullptr, nullptr, 0, 0, matrix);
    return SurfSrc{d_rec, c.ky, c.yoff, c.rv, c.gu, c.gv, c.bu};
}
void surf_to_rgb_launch(const SurfSrc& src, int B, int H, int W, unsigned char* out, hipStream_t s) {
    HP3D_LAUNCH(surf_to_rgb_kernel, dim3(grid_for((long)B * H * W)), dim3(256), 0, s, src, B, H, W, out);
}
void crop_and_resize_surf_launch(const SurfSrc& src, int n, int H, int W, const float* center, const float* scale, const int* idx, int K,
                                 int crop, float* out, hipStream_t s) {
    if (n < 1) return;
    const dim3 grid(grid_for((long)n * crop * crop)), block(256);
    if (idx) HP3D_LAUNCH(crop_and_resize_idx_surf_kernel, grid, block, 0, s, src, n, H, W, center, scale, idx, K, crop, out);
    else HP3D_LAUNCH(crop_and_resize_surf_kernel, grid, block, 0, s, src, n, H, W, center, scale, crop, out, K);
}
void downscale_surf_launch(const SurfSrc& src, const int* idx, int frames, int H, int W, int f, float* out, hipStream_t s) {
    if (frames < 1) return;
    if (f == 1) {
        const dim3 grid(grid_for((long)frames * H * W)), block(256);
        if (idx) HP3D_LAUNCH(preprocess_surf_kernel<true>, grid, block, 0, s, src, idx, frames, H, W, out);
        else HP3D_LAUNCH(preprocess_surf_kernel<false>, grid, block, 0, s, src, idx, frames, H, W, out);
        return;
    }
    const int Hd = (H + f - 1) / f, Wd = (W + f - 1) / f;
    const dim3 grid(grid_for((long)frames * Hd * Wd)), block(256);
    if (idx) {
        if (f == 2) HP3D_LAUNCH(downscale_surf_idx_kernel<2>, grid, block, 0, s, src, idx, frames, H, W, f, Hd, Wd, out);
        else if (f == 4) HP3D_LAUNCH(downscale_surf_idx_kernel<4>, grid, block, 0, s, src, idx, frames, H, W, f, Hd, Wd, out);
        else if (f == 8) HP3D_LAUNCH(downscale_surf_idx_kernel<8>, grid, block, 0, s, src, idx, frames, H, W, f, Hd, Wd, out);
        else HP3D_LAUNCH(downscale_surf_idx_kernel<0>, grid, block, 0, s, src, idx, frames, H, W, f, Hd, Wd, out);
    } else {
        if (f == 2) HP3D_LAUNCH(downscale_surf_kernel<2>, grid, block, 0, s, src, frames, H, W, f, Hd, Wd, out);
        else if (f == 4) HP3D_LAUNCH(downscale_surf_kernel<4>, grid, block, 0, s, src, frames, H, W, f, Hd, Wd, out);
        else if (f == 8) HP3D_LAUNCH(downscale_surf_kernel<8>, grid, block, 0, s, src, frames, H, W, f, Hd, Wd, out);
        else HP3D_LAUNCH(downscale_surf_kernel<0>, grid, block, 0, s, src, frames, H, W, f, Hd, Wd, out);
    }
}
void box_to_frame_launch(const float* center_d, const float* crop_size_d, int n, int f, float* center, float* crop_size, float* scale,
                         hipStream_t s) {
    HP3D_LAUNCH(box_to_frame_kernel, dim3(grid_for(n)), dim3(256), 0, s, center_d, crop_size_d, n, (float)f, (float)(f - 1) / 2.0f, center,
                crop_size, scale);
}
void box_to_detect_launch(const float* center, const float* scale, int n, int f, float* center_d, float* scale_d, hipStream_t s) {
    HP3D_LAUNCH(box_to_detect_kernel, dim3(grid_for(n)), dim3(256), 0, s, center, scale, n, (float)f, (float)(f - 1) / 2.0f, center_d, scale_d);
}
void argmax2d_launch(const float* x, int B, int H, int W, int C, int cs, int* out_rc, hipStream_t s) {
    HP3D_LAUNCH(argmax2d_kernel, dim3(C, B), dim3(256), 0, s, x, H, W, C, cs, out_rc);
}
