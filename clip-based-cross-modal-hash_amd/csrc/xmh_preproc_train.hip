// Training image transform on the GPU: the reference's
//     Compose([RandomHorizontalFlip(), RandomResizedCrop(r), ToTensor(), Normalize(mean, std)])
// (dataset/transformer_dataset.py:34-40) on a RAGGED batch of raw RGB uint8 photos, every image with its own crop box and flip,
// bit-exact with
//     Image.fromarray(a) [.transpose(FLIP_LEFT_RIGHT)] .crop((left, top, left + w, top + h)) .resize((r, r), Image.BILINEAR)
// followed by float32 ((u8 / 255) - mean) / std written channel-major.  The random draw stays on the host (a few numbers per
// image, xmh/dataset/preprocess.py); what the device gets is one packed pixel buffer and one descriptor per image.
//
// Three launches per batch, whatever B is, sized from host-known upper bounds (max crop height / width, r):
//   k_train_tables  Pillow's precompute_coeffs + normalize_coeffs_8bpc per (image, axis, output pixel), in double, in Pillow's
//                   order of operations: int32 taps with 22 fractional bits, (first input index, tap count) bounds
//   k_train_h       horizontal pass of the crop (flip folded into the source column) -> uint8 tmp [B][max_h][r][3]
//   k_train_v       vertical pass + normalise -> uint8 [B][r][r][3] and / or float [B][3][r][r]
// A pass whose crop dimension already equals r is a copy, as in Pillow (ImagingResample skips it).  The evaluation kernel beside
// this one (xmh_preproc.hip) shares one host-made table per (input size, output size) across a batch and resamples whole images
// with the bicubic filter; here the tables differ per image, so they are made where they are used.
// Every source coordinate is clamped into its image and every byte index into the pixel buffer (as k_scatter_rows clamps): a bad
// descriptor gives wrong pixels, never a read outside `pixels`.  The host checks the boxes before it launches anything.
#include "xmh_common.h"

// Pillow's host build has no FMA: a * b + c is two roundings.  File scope, so that it also holds for tri(), which is inlined into the
// table kernel with a product as its argument; the two resampling kernels are integer arithmetic plus the __f*_rn intrinsics.
#pragma clang fp contract(off)

namespace {

constexpr int kPrecisionBits = 32 - 8 - 2;
constexpr int kMaxSide = 1 << 16;                              // of a crop (table stride) and of r
constexpr int64_t kMaxImageSide = 1 << 20;                     // of an uploaded image: H * W * 3 stays far inside int64

__device__ __forceinline__ uint8_t clip8(int v) {
    v >>= kPrecisionBits;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

__device__ __forceinline__ int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

inline int taps_for(int in, int r) {                           // Pillow: (int)ceil(support) * 2 + 1, support = 1.0 * max(in / r, 1)
    const int c = in <= r ? 1 : (in + r - 1) / r;
    return 2 * c + 1;
}

// Pillow's bilinear_filter
__device__ __forceinline__ double tri(double x) {
    if (x < 0.0) x = -x;
    return x < 1.0 ? 1.0 - x : 0.0;
}

// one thread per (image, axis, output pixel)
__global__ __launch_bounds__(256) void k_train_tables(const xmh_crop_desc* __restrict__ desc, int64_t B, int r, int max_h, int max_w,
                                                      int ksw, int ksh, int32_t* __restrict__ bounds_w, int32_t* __restrict__ kk_w,
                                                      int32_t* __restrict__ bounds_h, int32_t* __restrict__ kk_h) {
    const int64_t total = B * 2 * r;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int xx = (int)(e % r);
        const int axis = (int)((e / r) & 1);                   // 0: columns (w), 1: rows (h)
        const int64_t b = e / (2 * (int64_t)r);
        const int raw = axis ? desc[b].h : desc[b].w;
        const int cap = axis ? max_h : max_w;
        const int in = raw < 1 ? 1 : (raw > cap ? cap : raw);
        if (in == r) continue;                                 // this pass is a copy
        const int ks = axis ? ksh : ksw;
        int32_t* bo = (axis ? bounds_h : bounds_w) + (b * r + xx) * 2;
        int32_t* k = (axis ? kk_h : kk_w) + (b * r + xx) * (int64_t)ks;
        const double scale = __ddiv_rn((double)in, (double)r);
        const double filterscale = scale < 1.0 ? 1.0 : scale;
        const double support = 1.0 * filterscale;
        const double ss = __ddiv_rn(1.0, filterscale);
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in) xmax = in;
        xmax -= xmin;
        if (xmax > ks) xmax = ks;                              // cannot happen for in <= cap; keeps a bad descriptor inside its table row
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) ww += tri((x + xmin - center + 0.5) * ss);      // left to right
        for (int x = 0; x < xmax; ++x) {
            double w = tri((x + xmin - center + 0.5) * ss);
            if (ww != 0.0) w = __ddiv_rn(w, ww);
            k[x] = w < 0.0 ? (int)(-0.5 + w * (double)(1 << kPrecisionBits)) : (int)(0.5 + w * (double)(1 << kPrecisionBits));
        }
        bo[0] = xmin;
        bo[1] = xmax;
    }
}

// horizontal: crop rows of the packed photos -> tmp [B][max_h][r][3]; one thread per tmp pixel, rows beyond an image's crop idle
__global__ __launch_bounds__(256) void k_train_h(const uint8_t* __restrict__ pixels, int64_t pixel_bytes, const xmh_crop_desc* __restrict__ desc,
                                                 int64_t B, int r, int max_h, int max_w, int ksw, const int32_t* __restrict__ bounds_w,
                                                 const int32_t* __restrict__ kk_w, uint8_t* __restrict__ tmp) {
    const int64_t total = B * max_h * r;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int xo = (int)(e % r);
        const int y = (int)((e / r) % max_h);
        const int64_t b = e / ((int64_t)r * max_h);
        const xmh_crop_desc d = desc[b];
        const int in_h = d.h < 1 ? 1 : (d.h > max_h ? max_h : d.h);
        if (y >= in_h) continue;
        const int in_w = d.w < 1 ? 1 : (d.w > max_w ? max_w : d.w);
        const int64_t H = clamp64(d.H, 1, kMaxImageSide), W = clamp64(d.W, 1, kMaxImageSide);
        const int64_t sy = clamp64((int64_t)d.top + y, 0, H - 1);
        const int64_t row = clamp64(d.offset, 0, pixel_bytes) + sy * W * 3;
        int xmin = xo, cnt = 1;
        const int32_t* k = nullptr;                            // in_w == r: the pass is a copy
        if (in_w != r) {
            xmin = bounds_w[(b * r + xo) * 2];
            cnt = bounds_w[(b * r + xo) * 2 + 1];
            k = kk_w + (b * r + xo) * (int64_t)ksw;
        }
        int s0 = 1 << (kPrecisionBits - 1), s1 = s0, s2 = s0;
        for (int t = 0; t < cnt; ++t) {
            int64_t sx = (int64_t)d.left + xmin + t;           // column of the flipped image
            if (d.flip) sx = W - 1 - sx;
            sx = clamp64(sx, 0, W - 1);
            const uint8_t* p = pixels + clamp64(row + sx * 3, 0, pixel_bytes - 3);
            const int w = k ? k[t] : (1 << kPrecisionBits);
            s0 += (int)p[0] * w;
            s1 += (int)p[1] * w;
            s2 += (int)p[2] * w;
        }
        uint8_t* o = tmp + e * 3;
        o[0] = clip8(s0); o[1] = clip8(s1); o[2] = clip8(s2);
    }
}

// vertical (+ normalise): tmp [B][max_h][r][3] -> u8 [B][r][r][3] and/or float [B][3][r][r]
__global__ __launch_bounds__(256) void k_train_v(const uint8_t* __restrict__ tmp, const xmh_crop_desc* __restrict__ desc, int64_t B, int r,
                                                 int max_h, int ksh, const int32_t* __restrict__ bounds_h, const int32_t* __restrict__ kk_h,
                                                 float m0, float m1, float m2, float d0, float d1, float d2,
                                                 uint8_t* __restrict__ out_u8, float* __restrict__ out_f) {
    const int64_t total = B * r * r;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int xo = (int)(e % r);
        const int yo = (int)((e / r) % r);
        const int64_t b = e / ((int64_t)r * r);
        const int raw_h = desc[b].h;
        const int in_h = raw_h < 1 ? 1 : (raw_h > max_h ? max_h : raw_h);
        int ymin = yo, cnt = 1;
        const int32_t* k = nullptr;                            // in_h == r: no vertical pass in Pillow either
        if (in_h != r) {
            ymin = bounds_h[(b * r + yo) * 2];
            cnt = bounds_h[(b * r + yo) * 2 + 1];
            k = kk_h + (b * r + yo) * (int64_t)ksh;
        }
        int s0 = 1 << (kPrecisionBits - 1), s1 = s0, s2 = s0;
        for (int t = 0; t < cnt; ++t) {
            int yy = ymin + t;
            yy = yy < 0 ? 0 : (yy > in_h - 1 ? in_h - 1 : yy);
            const uint8_t* p = tmp + ((b * max_h + yy) * r + xo) * 3;
            const int w = k ? k[t] : (1 << kPrecisionBits);
            s0 += (int)p[0] * w;
            s1 += (int)p[1] * w;
            s2 += (int)p[2] * w;
        }
        const uint8_t r0 = clip8(s0), r1 = clip8(s1), r2 = clip8(s2);
        if (out_u8) {
            uint8_t* o = out_u8 + e * 3;
            o[0] = r0; o[1] = r1; o[2] = r2;
        }
        if (out_f) {
            // ToTensor: float32(u8) / 255; Normalize: (x - mean) / std -- IEEE divisions, no reciprocal shortcuts (as k_resample_v)
            const int64_t plane = (int64_t)r * r;
            float* o = out_f + b * 3 * plane + (int64_t)yo * r + xo;
            o[0] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)r0, 255.0f), m0), d0);
            o[plane] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)r1, 255.0f), m1), d1);
            o[2 * plane] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)r2, 255.0f), m2), d2);
        }
    }
}

inline unsigned grid_for(int64_t work) {
    int64_t g = xmh::ceil_div(work, 256);
    const int64_t cap = (int64_t)xmh::device_cu_count() * 16;
    return (unsigned)(g > cap ? cap : (g < 1 ? 1 : g));
}

inline size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

struct TrainWs {
    size_t bounds_w, bounds_h, kk_w, kk_h, tmp, total;
    int ksw, ksh;
};

inline bool shape_ok(int64_t B, int max_h, int max_w, int r) {
    return B >= 0 && B <= (1 << 20) && max_h >= 1 && max_h <= kMaxSide && max_w >= 1 && max_w <= kMaxSide && r >= 1 && r <= kMaxSide;
}

inline TrainWs layout(int64_t B, int max_h, int max_w, int r) {
    TrainWs w;
    w.ksw = taps_for(max_w, r);
    w.ksh = taps_for(max_h, r);
    size_t at = 0;
    const size_t rows = (size_t)B * (size_t)r;
    w.bounds_w = at; at += up256(rows * 2 * sizeof(int32_t));
    w.bounds_h = at; at += up256(rows * 2 * sizeof(int32_t));
    w.kk_w = at; at += up256(rows * (size_t)w.ksw * sizeof(int32_t));
    w.kk_h = at; at += up256(rows * (size_t)w.ksh * sizeof(int32_t));
    w.tmp = at; at += up256((size_t)B * (size_t)max_h * (size_t)r * 3);
    w.total = at;
    return w;
}

}  // namespace

extern "C" size_t xmh_image_preprocess_train_ws_bytes(int64_t B, int max_h, int max_w, int r) {
    if (!shape_ok(B, max_h, max_w, r)) return 0;
    return layout(B, max_h, max_w, r).total;
}

extern "C" int xmh_image_preprocess_train_u8(const uint8_t* pixels, int64_t pixel_bytes, const xmh_crop_desc* desc, int64_t B, int max_h,
                                             int max_w, int r, const float* mean3_host, const float* std3_host, void* workspace,
                                             size_t workspace_bytes, uint8_t* resized_u8, float* out_chw, xmh_stream_t stream) {
    XMH_RANGE("xmh_image_preprocess_train_u8");
    if (!shape_ok(B, max_h, max_w, r))
        return xmh::fail(XMH_EINVAL, "xmh_image_preprocess_train_u8: bad shape (B %lld, max crop %d x %d, r %d)", (long long)B, max_h, max_w, r);
    if (B == 0) return XMH_OK;
    if (!pixels || !desc || !workspace || (!resized_u8 && !out_chw)) return xmh::fail(XMH_EINVAL, "xmh_image_preprocess_train_u8: null pointer");
    if (pixel_bytes < 3) return xmh::fail(XMH_EINVAL, "xmh_image_preprocess_train_u8: pixel buffer of %lld bytes", (long long)pixel_bytes);
    if (out_chw && (!mean3_host || !std3_host)) return xmh::fail(XMH_EINVAL, "xmh_image_preprocess_train_u8: mean/std missing");
    const TrainWs w = layout(B, max_h, max_w, r);
    if (workspace_bytes < w.total)
        return xmh::fail(XMH_ENOMEM, "xmh_image_preprocess_train_u8: workspace of %zu bytes, %zu needed", workspace_bytes, w.total);
    hipStream_t st = xmh::as_stream(stream);
    uint8_t* base = static_cast<uint8_t*>(workspace);
    int32_t* bounds_w = reinterpret_cast<int32_t*>(base + w.bounds_w);
    int32_t* bounds_h = reinterpret_cast<int32_t*>(base + w.bounds_h);
    int32_t* kk_w = reinterpret_cast<int32_t*>(base + w.kk_w);
    int32_t* kk_h = reinterpret_cast<int32_t*>(base + w.kk_h);
    uint8_t* tmp = base + w.tmp;
    // one ProfScope per launch: xmh_prof_read gives each kernel's time and how often it ran (once per call, whatever B is)
    {
        xmh::ProfScope prof("train_tf_tables", st);
        hipLaunchKernelGGL(k_train_tables, dim3(grid_for(B * 2 * r)), dim3(256), 0, st, desc, B, r, max_h, max_w, w.ksw, w.ksh, bounds_w, kk_w,
                           bounds_h, kk_h);
    }
    XMH_LAUNCH_CHECK("xmh_image_preprocess_train_u8 tables");
    {
        xmh::ProfScope prof("train_tf_h", st);
        hipLaunchKernelGGL(k_train_h, dim3(grid_for(B * max_h * r)), dim3(256), 0, st, pixels, pixel_bytes, desc, B, r, max_h, max_w, w.ksw,
                           bounds_w, kk_w, tmp);
    }
    XMH_LAUNCH_CHECK("xmh_image_preprocess_train_u8 horizontal");
    const float m0 = out_chw ? mean3_host[0] : 0.f, m1 = out_chw ? mean3_host[1] : 0.f, m2 = out_chw ? mean3_host[2] : 0.f;
    const float d0 = out_chw ? std3_host[0] : 1.f, d1 = out_chw ? std3_host[1] : 1.f, d2 = out_chw ? std3_host[2] : 1.f;
    {
        xmh::ProfScope prof("train_tf_v", st);
        hipLaunchKernelGGL(k_train_v, dim3(grid_for(B * r * r)), dim3(256), 0, st, tmp, desc, B, r, max_h, w.ksh, bounds_h, kk_h, m0, m1, m2, d0,
                           d1, d2, resized_u8, out_chw);
    }
    XMH_LAUNCH_CHECK("xmh_image_preprocess_train_u8 vertical");
    return XMH_OK;
}
