// mpt_svgf.h — spatiotemporal variance-guided filtering (included by mpt_hip.hip after mpt_temporal.h):
//   k_sv_reproject   step A: carries the demodulated illumination and its luminance moments from the history's camera to the current one
//   k_sv_variance    step B: the variance of the accumulated mean, from the moments (n >= 4) or from a 7 x 7 window of them (n < 4)
//   k_sv_level       step C: one a-trous level over (x, V) whose luminance stop is the prefiltered variance
//   k_sv_modulate    iterations = 0: the history times the albedo
//   k_sv_pack        caller-supplied guide arrays -> the packed history guide (mpt_svgf_image)
// The stage is specified exactly in include/mpt.h (mpt_svgf_params) and restated in numpy in tests/svgf_ref.py, which follows the
// tap order and the operation order of these kernels; DESIGN.md §13 has the layout.
// Step A: only + - * / sqrt floor and comparisons, one IEEE operation each (-ffp-contract=off): the device and numpy agree bit for bit.
#pragma once

// History guide, 16 bytes (one load): (normal facing the ray, t) with the class in t: t for a surface, -t for an emitter (a hit
// distance is > 0), +inf for a miss.  The taps of steps B and C use the denoiser's packed guide (MPT_DN_SKIP for classes 1 / 2).
#define MPT_SV_WIN 3             // step B: the window is (2 * 3 + 1)^2
#define MPT_SV_WIN_T (MPT_DN_TILE + 2 * MPT_SV_WIN)

struct SvFrame {
    const float4* color;     // this frame's colour before division by `samples`
    const float4* ad;        // current guide: (albedo, t)
    const float4* nc;        //                (normal, class)
    const float4* hist_in;   // (X rgb, n), (M1, M2) and the guide of the history's frame — unused by MPT_TP_NONE
    const float2* mom_in;
    const float4* guide_in;
    float4* hist_out;
    float2* mom_out;
    float4* guide_out;
    unsigned long long* n_reset;
    uint32_t W, H;
    float fW, fH;
    float samples;
    F3 cam, first, vu, vv;
    F3 cam_h, vu_h, vv_h;
    F3 nn, fc;
    float fcnn, uu, vvl;
    float depth_tol, normal_thr, min_weight, max_history;
};

__device__ __forceinline__ float sv_guide_t(float cls, float t) { return cls == 2.0f ? MPT_TP_MISS_T : cls == 1.0f ? -t : t; }

__global__ __launch_bounds__(256) void k_sv_pack(const float4* ad, const float4* nc, uint32_t n, float4* guide) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 a = ad[i], b = nc[i];
    guide[i] = make_float4(b.x, b.y, b.z, sv_guide_t(b.w, a.w));
}

// k_tp_reproject's launch shape and arithmetic; a tap must also be of the pixel's class, and the moments ride along.
template <int MODE>
__global__ __launch_bounds__(256) void k_sv_reproject(SvFrame T) {
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t px = blockIdx.x * MPT_DN_TILE + (wave & 1u) * 8u + (lane & 7u);
    const uint32_t py = blockIdx.y * MPT_DN_TILE + (wave >> 1) * 8u + (lane >> 3);
    const bool inside = px < T.W && py < T.H;
    bool reset = false;
    if (inside) {
        const size_t p = (size_t)py * T.W + px;
        const float4 cs = T.color[p], a = T.ad[p], g = T.nc[p];
        const bool surf = g.w == 0.0f, hit = g.w != 2.0f, emit = g.w == 1.0f;
        const float ar = surf ? fmaxf(a.x, 1e-3f) : 1.0f, ag = surf ? fmaxf(a.y, 1e-3f) : 1.0f, ab = surf ? fmaxf(a.z, 1e-3f) : 1.0f;
        const float xr = (cs.x / T.samples) / ar, xg = (cs.y / T.samples) / ag, xb = (cs.z / T.samples) / ab;
        const float l = dn_lum(xr, xg, xb);
        const float ll = l * l;
        T.guide_out[p] = make_float4(g.x, g.y, g.z, sv_guide_t(g.w, a.w));
        float sr = 0.0f, sg = 0.0f, sb = 0.0f, sn = 0.0f, s1 = 0.0f, s2 = 0.0f, sw = 0.0f;
        if (MODE == MPT_TP_SAME) {
            const float4 h = T.hist_in[p];
            const float2 m = T.mom_in[p];
            sr = h.x, sg = h.y, sb = h.z, sn = h.w, s1 = m.x, s2 = m.y, sw = 1.0f;
        } else if (MODE == MPT_TP_MOVED) {
            const float uvx = ((float)px + 0.5f) / T.fW, uvy = ((float)py + 0.5f) / T.fH;
            const F3 dv = (T.first + uvx * T.vu + uvy * T.vv) - T.cam;
            const F3 d = dv * (1.0f / sqrtf(tp_dot(dv, dv)));
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
                        const bool ok = hit ? (qhit && (gq.w < 0.0f) == emit && fabsf(fabsf(gq.w) - rl) <= tol &&
                                               tp_dot(n, F3{gq.x, gq.y, gq.z}) >= T.normal_thr)
                                            : !qhit;
                        if (!ok) continue;
                        const float w = (i ? ax : 1.0f - ax) * (j ? ay : 1.0f - ay);
                        const float4 h = T.hist_in[qi];
                        const float2 m = T.mom_in[qi];
                        sr = sr + w * h.x;
                        sg = sg + w * h.y;
                        sb = sb + w * h.z;
                        sn = sn + w * h.w;
                        s1 = s1 + w * m.x;
                        s2 = s2 + w * m.y;
                        sw = sw + w;
                    }
                }
            }
        }
        reset = MODE == MPT_TP_NONE || !(sw >= T.min_weight);
        if (reset) {
            T.hist_out[p] = make_float4(xr, xg, xb, 1.0f);
            T.mom_out[p] = make_float2(l, ll);
        } else {
            const float hr = sr / sw, hg = sg / sw, hb = sb / sw, m = sn / sw, m1 = s1 / sw, m2 = s2 / sw;
            const float n = fminf(m + 1.0f, T.max_history);
            T.hist_out[p] = make_float4(hr + (xr - hr) / n, hg + (xg - hg) / n, hb + (xb - hb) / n, n);
            T.mom_out[p] = make_float2(m1 + (l - m1) / n, m2 + (ll - m2) / n);
        }
    }
    const unsigned long long lost = __ballot(reset);
    if (lane == 0 && lost) atomicAdd(T.n_reset, (unsigned long long)__popcll(lost));
}

static const void* sv_reproject_kernel(int mode) {
    return mode == MPT_TP_NONE ? (const void*)k_sv_reproject<MPT_TP_NONE>
           : mode == MPT_TP_SAME ? (const void*)k_sv_reproject<MPT_TP_SAME> : (const void*)k_sv_reproject<MPT_TP_MOVED>;
}

// ---- step B ----------------------------------------------------------------------------------------------------------------------
// xv = (X rgb, V_0).  A workgroup stages the 22 x 22 window tile of (M1, M2) and the guide only if one of its surface pixels has a
// history shorter than 4: after a few frames that is the rim of the disocclusions.
struct SvVariance {
    const float4* hist;    // (X rgb, n)
    const float2* mom;     // (M1, M2)
    const float4* guide;   // the denoiser's packed guide of the current frame
    float4* xv;
    uint32_t W, H;
    float sigma_n, sigma_z;
};

__global__ __launch_bounds__(256) void k_sv_variance(SvVariance S) {
    __shared__ float4 g_lds[MPT_SV_WIN_T * MPT_SV_WIN_T];
    __shared__ float2 m_lds[MPT_SV_WIN_T * MPT_SV_WIN_T];
    const int W = (int)S.W, H = (int)S.H;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int lx = (wave & 1) * 8 + (lane & 7), ly = (wave >> 1) * 8 + (lane >> 3);
    const int px = blockIdx.x * MPT_DN_TILE + lx, py = blockIdx.y * MPT_DN_TILE + ly;
    const bool inside = px < W && py < H;
    const size_t p = inside ? (size_t)py * W + px : 0;
    float4 h = make_float4(0.0f, 0.0f, 0.0f, 0.0f), gp = make_float4(0.0f, 0.0f, 0.0f, MPT_DN_SKIP);
    float2 m = make_float2(0.0f, 0.0f);
    if (inside) {
        h = S.hist[p];
        gp = S.guide[p];
        m = S.mom[p];
    }
    const bool surf = gp.w >= 0.0f;
    const bool spatial = surf && !(h.w >= 4.0f);
    if (__syncthreads_or(spatial)) {
        const int T = MPT_SV_WIN_T;
        const int ox = blockIdx.x * MPT_DN_TILE - MPT_SV_WIN, oy = blockIdx.y * MPT_DN_TILE - MPT_SV_WIN;
        for (int k = threadIdx.x; k < T * T; k += blockDim.x) {
            const int gx = ox + k % T, gy = oy + k / T;
            float4 g = make_float4(0.0f, 0.0f, 0.0f, MPT_DN_SKIP);
            float2 mq = make_float2(0.0f, 0.0f);
            if (gx >= 0 && gy >= 0 && gx < W && gy < H) {
                const size_t q = (size_t)gy * W + gx;
                g = S.guide[q];
                if (g.w >= 0.0f) mq = S.mom[q];
            }
            g_lds[k] = g;
            m_lds[k] = mq;
        }
        __syncthreads();
    }
    if (!inside) return;
    float v = 0.0f;
    if (surf) {
        if (!spatial) {
            v = fmaxf(0.0f, m.y - m.x * m.x) / h.w;
        } else {
            const int T = MPT_SV_WIN_T;
            const int cp = (ly + MPT_SV_WIN) * T + (lx + MPT_SV_WIN);
            const float den_z = S.sigma_z * gp.w;
            float s1 = 0.0f, s2 = 0.0f, sw = 0.0f;
            for (int dy = -MPT_SV_WIN; dy <= MPT_SV_WIN; ++dy) {
                for (int dx = -MPT_SV_WIN; dx <= MPT_SV_WIN; ++dx) {
                    const int cq = cp + dy * T + dx;
                    const float4 gq = g_lds[cq];
                    if (gq.w < 0.0f) continue;
                    const float2 mq = m_lds[cq];
                    float w = 1.0f;
                    if (dx != 0 || dy != 0) {
                        const float nd = (gp.x * gq.x + gp.y * gq.y) + gp.z * gq.z;
                        const float wn = powf(fmaxf(0.0f, nd), S.sigma_n);
                        const float wz = expf(-fabsf(gp.w - gq.w) / den_z);
                        w = wn * wz;
                    }
                    s1 = s1 + w * mq.x;
                    s2 = s2 + w * mq.y;
                    sw = sw + w;
                }
            }
            const float e1 = s1 / sw;
            v = fmaxf(0.0f, s2 / sw - e1 * e1) / h.w;
        }
    }
    S.xv[p] = make_float4(h.x, h.y, h.z, v);
}

// ---- step C ----------------------------------------------------------------------------------------------------------------------
struct SvLevel {
    const float4* xin;     // (x_i rgb, V_i)
    const float4* guide;   // the denoiser's packed per-tap guide
    const float4* ad;      // LAST: (albedo, t), remodulates
    const float4* hist;    // LAST: (X rgb, n): the output of classes 1 / 2 and every pixel's alpha
    float4* xout;          // (x_{i+1} rgb, V_{i+1}), or LAST: the filtered rgba
    float4* feedback;      // level 0 with feedback: the illumination history, rgb <- x_1 for surface pixels (null otherwise)
    uint32_t W, H;
    uint32_t step;         // s = 2^i
    float sigma_n, sigma_z, sigma_l;
};

// 5 x 5 taps q = p + s (dx, dy), dy outer, as k_dn_level.  g_p: the {1,2,1}^2 / 16 mean of V_i over the ADJACENT surface pixels.
// Weight: (h[dx] * h[dy]) * ((wn * wz) * wl), wl = exp(-|lum(x_p) - lum(x_q)| / (sigma_l * sqrt(g_p) + MPT_SVGF_EPSILON)); the centre's is
// h[0]^2.  x_{i+1} = (sum w x) / (sum w); V_{i+1} = (sum (w * w) V) / ((sum w) * (sum w)).
template <bool LDS, bool LAST>
__global__ __launch_bounds__(256) void k_sv_level(SvLevel L) {
    extern __shared__ float4 sv_lds[];   // [T*T] (x, V) then [T*T] guide, T = 16 + 4s
    const int s = (int)L.step, W = (int)L.W, H = (int)L.H;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int lx = (wave & 1) * 8 + (lane & 7), ly = (wave >> 1) * 8 + (lane >> 3);
    const int px = blockIdx.x * MPT_DN_TILE + lx, py = blockIdx.y * MPT_DN_TILE + ly;
    const int T = MPT_DN_TILE + 4 * s;
    if (LDS) {
        const int ox = blockIdx.x * MPT_DN_TILE - 2 * s, oy = blockIdx.y * MPT_DN_TILE - 2 * s;
        for (int k = threadIdx.x; k < T * T; k += blockDim.x) {
            const int gx = ox + k % T, gy = oy + k / T;
            float4 x = make_float4(0.0f, 0.0f, 0.0f, 0.0f), g = make_float4(0.0f, 0.0f, 0.0f, MPT_DN_SKIP);
            if (gx >= 0 && gy >= 0 && gx < W && gy < H) {
                const size_t q = (size_t)gy * W + gx;
                g = L.guide[q];
                if (g.w >= 0.0f) x = L.xin[q];
            }
            sv_lds[k] = x;
            sv_lds[T * T + k] = g;
        }
        __syncthreads();
    }
    if (px >= W || py >= H) return;
    const size_t p = (size_t)py * W + px;
    const int cp = LDS ? (ly + 2 * s) * T + (lx + 2 * s) : 0;
    const float4 gp = LDS ? sv_lds[T * T + cp] : L.guide[p];
    if (gp.w < 0.0f) {   // emitter or sky: the accumulated radiance, never filtered
        if (LAST) L.xout[p] = L.hist[p];
        return;
    }
    const float4 xp = LDS ? sv_lds[cp] : L.xin[p];
    const float lp = dn_lum(xp.x, xp.y, xp.z);
    const float k3[3] = {0.25f, 0.5f, 0.25f};
    float gs = 0.0f, gw = 0.0f;
    for (int dy = -1; dy <= 1; ++dy) {
        const int qy = py + dy;
        if (!LDS && (qy < 0 || qy >= H)) continue;
        for (int dx = -1; dx <= 1; ++dx) {
            const int qx = px + dx;
            float vq;
            if (LDS) {
                const int cq = cp + dy * T + dx;
                if (sv_lds[T * T + cq].w < 0.0f) continue;
                vq = sv_lds[cq].w;
            } else {
                if (qx < 0 || qx >= W) continue;
                const size_t q = (size_t)qy * W + qx;
                if (L.guide[q].w < 0.0f) continue;
                vq = L.xin[q].w;
            }
            const float k = k3[dx + 1] * k3[dy + 1];
            gs = gs + k * vq;
            gw = gw + k;
        }
    }
    const float den_l = L.sigma_l * sqrtf(gs / gw) + MPT_SVGF_EPSILON;
    const float hk[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    const float den_z = (L.sigma_z * gp.w) * (float)s;
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sv = 0.0f, sw = 0.0f;
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = py + s * dy;
        if (!LDS && (qy < 0 || qy >= H)) continue;
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = px + s * dx;
            float4 gq, xq;
            if (LDS) {
                const int cq = cp + s * (dy * T + dx);
                gq = sv_lds[T * T + cq];
                if (gq.w < 0.0f) continue;
                xq = sv_lds[cq];
            } else {
                if (qx < 0 || qx >= W) continue;
                const size_t q = (size_t)qy * W + qx;
                gq = L.guide[q];
                if (gq.w < 0.0f) continue;
                xq = L.xin[q];
            }
            const float k = hk[dx + 2] * hk[dy + 2];
            float w;
            if (dx == 0 && dy == 0) {
                w = k;
            } else {
                const float nd = (gp.x * gq.x + gp.y * gq.y) + gp.z * gq.z;
                const float wn = powf(fmaxf(0.0f, nd), L.sigma_n);
                const float wz = expf(-fabsf(gp.w - gq.w) / den_z);
                const float wl = expf(-fabsf(lp - dn_lum(xq.x, xq.y, xq.z)) / den_l);
                w = k * ((wn * wz) * wl);
            }
            sr = sr + w * xq.x;
            sg = sg + w * xq.y;
            sb = sb + w * xq.z;
            sv = sv + (w * w) * xq.w;
            sw = sw + w;
        }
    }
    const float r = sr / sw, g = sg / sw, b = sb / sw;
    if (L.feedback) {
        const float4 h = L.feedback[p];
        L.feedback[p] = make_float4(r, g, b, h.w);
    }
    if (LAST) {
        const float4 a = L.ad[p];
        L.xout[p] = make_float4(r * fmaxf(a.x, 1e-3f), g * fmaxf(a.y, 1e-3f), b * fmaxf(a.z, 1e-3f), L.hist[p].w);
    } else {
        L.xout[p] = make_float4(r, g, b, sv / (sw * sw));
    }
}

template <bool LDS>
static const void* sv_level_kernel(bool last) {
    return last ? (const void*)k_sv_level<LDS, true> : (const void*)k_sv_level<LDS, false>;
}

// iterations = 0: X * a for a surface pixel, X for the others; alpha = n
__global__ __launch_bounds__(256) void k_sv_modulate(const float4* hist, const float4* ad, const float4* guide, uint32_t n, float4* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 h = hist[i];
    if (guide[i].w < 0.0f) {
        out[i] = h;
        return;
    }
    const float4 a = ad[i];
    out[i] = make_float4(h.x * fmaxf(a.x, 1e-3f), h.y * fmaxf(a.y, 1e-3f), h.z * fmaxf(a.z, 1e-3f), h.w);
}
