// mpt_temporal.h — temporal accumulation (included by mpt_hip.hip after mpt_denoise.h):
//   k_tp_reproject   carries the accumulated image from the history's camera to the current one and blends this frame's colour in
//   k_tp_pack        caller-supplied guide arrays -> the packed history guide (mpt_temporal_image)
// The stage is specified exactly in include/mpt.h (mpt_temporal_params) and restated in numpy in tests/temporal_ref.py, which
// follows the tap order and the operation order of k_tp_reproject; DESIGN.md §12 has the layout and the measured times.
// Only + - * / sqrt floor and comparisons, one IEEE operation each (-ffp-contract=off): the device and numpy agree bit for bit.
#pragma once

// History guide, 16 bytes (one load): (normal facing the ray, hit distance t) for a hit of class 0 or 1, t = +inf for a miss.
#define MPT_TP_MISS_T (__builtin_inff())
enum { MPT_TP_NONE = 0,     // no history: every pixel is reset
       MPT_TP_SAME = 1,     // the history's camera is the current one bit for bit: the only tap is the pixel itself
       MPT_TP_MOVED = 2 };  // reproject

// In the order of mpt_denoise.h (dn_lum): (a.x b.x + a.y b.y) + a.z b.z
__host__ __device__ __forceinline__ float tp_dot(F3 a, F3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

// Everything that does not depend on the pixel, computed on the host in float32 by the expressions of include/mpt.h and passed by
// value: it lives in SGPRs.
struct TpFrame {
    const float4* color;     // this frame's colour before division by `samples`
    const float4* ad;        // current guide: (albedo, t)
    const float4* nc;        //                (normal, class)
    const float4* hist_in;   // history (rgb, n) and its guide, at the history's camera — unused by MPT_TP_NONE
    const float4* guide_in;
    float4* hist_out;        // the new history and its guide (the current guide, packed)
    float4* guide_out;
    unsigned long long* n_reset;   // pixels that lost (or had no) history
    uint32_t W, H;
    float fW, fH;
    float samples;           // divisor of `color` (1 for FRAME and mpt_temporal_image: x / 1 is x)
    F3 cam, first, vu, vv;   // the current camera
    F3 cam_h, vu_h, vv_h;    // the history's camera: position, viewport vectors,
    F3 nn, fc;               // nn = cross(vu', vv'), fc = first' - cam',
    float fcnn, uu, vvl;     // dot(fc, nn), dot(vu', vu'), dot(vv', vv')
    float depth_tol, normal_thr, min_weight, max_history;
};

__global__ __launch_bounds__(256) void k_tp_pack(const float4* ad, const float4* nc, uint32_t n, float4* guide) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 a = ad[i], b = nc[i];
    guide[i] = make_float4(b.x, b.y, b.z, b.w == 2.0f ? MPT_TP_MISS_T : a.w);
}

// One thread per pixel, a 16 x 16 tile per workgroup as four 8 x 8 sub-tiles, one per wave (the denoiser's launch shape): the four
// taps of a wave fall into a few cache lines of the history and of its guide, read through L2.
template <int MODE>
__global__ __launch_bounds__(256) void k_tp_reproject(TpFrame T) {
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t px = blockIdx.x * MPT_DN_TILE + (wave & 1u) * 8u + (lane & 7u);
    const uint32_t py = blockIdx.y * MPT_DN_TILE + (wave >> 1) * 8u + (lane >> 3);
    const bool inside = px < T.W && py < T.H;
    bool reset = false;
    if (inside) {
        const size_t p = (size_t)py * T.W + px;
        const float4 cs = T.color[p], a = T.ad[p], g = T.nc[p];
        const float cr = cs.x / T.samples, cg = cs.y / T.samples, cb = cs.z / T.samples;
        const bool hit = g.w != 2.0f;
        T.guide_out[p] = make_float4(g.x, g.y, g.z, hit ? a.w : MPT_TP_MISS_T);
        float sr = 0.0f, sg = 0.0f, sb = 0.0f, sn = 0.0f, sw = 0.0f;
        if (MODE == MPT_TP_SAME) {
            const float4 h = T.hist_in[p];
            sr = h.x, sg = h.y, sb = h.z, sn = h.w, sw = 1.0f;
        } else if (MODE == MPT_TP_MOVED) {
            const float uvx = ((float)px + 0.5f) / T.fW, uvy = ((float)py + 0.5f) / T.fH;
            const F3 dv = (T.first + uvx * T.vu + uvy * T.vv) - T.cam;
            const F3 d = dv * (1.0f / sqrtf(tp_dot(dv, dv)));   // normalize3, with the division written out
            const F3 r = hit ? (T.cam + a.w * d) - T.cam_h : d;
            const float s = T.fcnn / tp_dot(r, T.nn);
            const F3 q = s * r - T.fc;
            const float u = tp_dot(q, T.vu_h) / T.uu, v = tp_dot(q, T.vv_h) / T.vvl;
            const float fx = u * T.fW - 0.5f, fy = v * T.fH - 0.5f;
            if (s > 0.0f && s < __builtin_inff() && fx >= -1.0f && fx < T.fW && fy >= -1.0f && fy < T.fH) {
                const float flx = floorf(fx), fly = floorf(fy);
                const int x0 = (int)flx, y0 = (int)fly;
                const float ax = fx - flx, ay = fy - fly;
                const float rl = sqrtf(tp_dot(r, r));
                const float tol = T.depth_tol * rl;
                const F3 n = F3{g.x, g.y, g.z};
#pragma unroll
                for (int j = 0; j < 2; ++j) {
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const int qx = x0 + i, qy = y0 + j;
                        if (qx < 0 || qy < 0 || qx >= (int)T.W || qy >= (int)T.H) continue;
                        const size_t qi = (size_t)qy * T.W + (size_t)qx;
                        const float4 gq = T.guide_in[qi];
                        const bool qhit = gq.w < __builtin_inff();
                        const bool ok = hit ? (qhit && fabsf(gq.w - rl) <= tol && tp_dot(n, F3{gq.x, gq.y, gq.z}) >= T.normal_thr) : !qhit;
                        if (!ok) continue;
                        const float w = (i ? ax : 1.0f - ax) * (j ? ay : 1.0f - ay);
                        const float4 h = T.hist_in[qi];
                        sr = sr + w * h.x;
                        sg = sg + w * h.y;
                        sb = sb + w * h.z;
                        sn = sn + w * h.w;
                        sw = sw + w;
                    }
                }
            }
        }
        reset = MODE == MPT_TP_NONE || !(sw >= T.min_weight);
        if (reset) {
            T.hist_out[p] = make_float4(cr, cg, cb, 1.0f);
        } else {
            const float hr = sr / sw, hg = sg / sw, hb = sb / sw, m = sn / sw;
            const float n = fminf(m + 1.0f, T.max_history);
            T.hist_out[p] = make_float4(hr + (cr - hr) / n, hg + (cg - hg) / n, hb + (cb - hb) / n, n);
        }
    }
    const unsigned long long lost = __ballot(reset);
    if (lane == 0 && lost) atomicAdd(T.n_reset, (unsigned long long)__popcll(lost));
}

static const void* tp_kernel(int mode) {
    return mode == MPT_TP_NONE ? (const void*)k_tp_reproject<MPT_TP_NONE>
           : mode == MPT_TP_SAME ? (const void*)k_tp_reproject<MPT_TP_SAME> : (const void*)k_tp_reproject<MPT_TP_MOVED>;
}
