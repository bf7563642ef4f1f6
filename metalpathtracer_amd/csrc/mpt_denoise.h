// mpt_denoise.h — the on-device denoiser (included by mpt_hip.hip after mpt_kernels.h):
//   k_dn_guide   first-hit guide buffers: one pixel-centre ray per pixel through the reference-order closest-hit walk
//   k_dn_pack    caller-supplied guide arrays -> the packed per-tap guide (mpt_denoise_image)
//   k_dn_level   one level of the edge-avoiding a-trous filter (Dammertz et al. 2010) in demodulated-irradiance space
//   k_dn_copy    iterations = 0: the input colour, unchanged
// The filter is specified exactly in include/mpt.h (mpt_denoise_params) and restated in numpy in tests/denoise_ref.py, which
// follows the tap order and the operation order of k_dn_level; DESIGN.md "Denoiser" has the layout and the measured times.
#pragma once

// Per-tap guide, 16 bytes (one load): (shading normal xyz, hit distance t) for a surface pixel (class 0), w = -1 for every other
// class — those pixels are never used as taps and never filtered.  A surface's t is a hit distance, so it is > 0.
#define MPT_DN_SKIP (-1.0f)
#define MPT_DN_TILE 16          // a workgroup of 256 threads filters / traces a 16 x 16 pixel tile (four 8 x 8 tiles, one per wave)
#define MPT_DN_LDS_MAX_STEP 4   // steps 1, 2, 4 stage the tile and its 2*s halo in LDS (<= 32 KiB); larger steps read taps from L2 / MALL

// Rec. 709 luminance, in this order (tests/denoise_ref.py: lum)
__device__ __forceinline__ float dn_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// ---- guide pass ------------------------------------------------------------------------------------------------------------
// gen_primary with zero jitter: uv = ((px + 0.5) / W, (py + 0.5) / H), dir = normalize(first + uvx * vu + uvy * vv - cam).
// ad = (albedo rgb, t), nc = (normal facing the ray, class), prim = caller's id (-1 on a miss), guide = the packed per-tap guide.
// Class: 0 surface, 1 emissive material (emissionPower > 0), 2 miss.  A miss stores albedo 0, t = +inf, normal 0.
__global__ __launch_bounds__(256) void k_dn_guide(SceneDev sc, F3 cam, F3 first, F3 vu, F3 vv, float fW, float fH, uint32_t W,
                                                  uint32_t H, float4* ad, float4* nc, int* prim_out, float4* guide) {
    extern __shared__ float4 lds_nodes[];
    stage_nodes(sc, lds_nodes);
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t px = blockIdx.x * MPT_DN_TILE + (wave & 1u) * 8u + (lane & 7u);
    const uint32_t py = blockIdx.y * MPT_DN_TILE + (wave >> 1) * 8u + (lane >> 3);
    if (px >= W || py >= H) return;
    const float uvx = ((float)px + 0.5f) / fW, uvy = ((float)py + 0.5f) / fH;
    const F3 o = cam, d = normalize3((first + uvx * vu + uvy * vv) - cam);
    float t;
    int prim;
    WorkCount wc = {};
    closest_hit<false, false>(sc, (LdsNodes)lds_nodes, o, d, t, prim, wc);
    const size_t i = (size_t)py * W + px;
    if (prim < 0) {
        ad[i] = make_float4(0.0f, 0.0f, 0.0f, t);
        nc[i] = make_float4(0.0f, 0.0f, 0.0f, 2.0f);
        prim_out[i] = -1;
        guide[i] = make_float4(0.0f, 0.0f, 0.0f, MPT_DN_SKIP);
        return;
    }
    const HitInfo h = finish_hit(sc, (LdsNodes)lds_nodes, o, d, t, prim);
    const float4 m0 = sc.mats[2 * h.mat], m1 = sc.mats[2 * h.mat + 1];
    const bool emissive = m1.w > 0.0f;
    ad[i] = make_float4(m0.x, m0.y, m0.z, t);
    nc[i] = make_float4(h.normal.x, h.normal.y, h.normal.z, emissive ? 1.0f : 0.0f);
    prim_out[i] = h.orig_id;
    guide[i] = make_float4(h.normal.x, h.normal.y, h.normal.z, emissive ? MPT_DN_SKIP : t);
}

__global__ __launch_bounds__(256) void k_dn_pack(const float4* ad, const float4* nc, uint32_t n, float4* guide) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 a = ad[i], b = nc[i];
    guide[i] = make_float4(b.x, b.y, b.z, b.w == 0.0f ? a.w : MPT_DN_SKIP);
}

__global__ __launch_bounds__(256) void k_dn_copy(const float4* color, float samples, uint32_t n, float4* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 c = color[i];
    out[i] = make_float4(c.x / samples, c.y / samples, c.z / samples, c.w / samples);
}

// ---- one filter level -------------------------------------------------------------------------------------------------------
struct DnLevel {
    const float4* color;   // the input colour before division by `samples` (FIRST: demodulated into x0; LAST: pass-through pixels, alpha)
    const float4* ad;      // (albedo, t): FIRST demodulates by it, LAST remodulates
    const float4* guide;   // packed per-tap guide
    const float4* xin;     // (x_i rgb, luminance of x_i) — unused by FIRST
    float4* xout;          // (x_{i+1} rgb, its luminance), or LAST: the denoised rgba
    uint32_t W, H;
    uint32_t step;         // s = 2^i
    float samples;         // divisor of `color` (1 for FRAME and mpt_denoise_image: x / 1 is x)
    float sigma_n;         // the normal exponent
    float sigma_z;         // depth: exp(-|t_p - t_q| / ((sigma_z * t_p) * s))
    float sigma_l;         // luminance of this level: exp(-|l_p - l_q| / (sigma_luminance * 2^-i)), the product already taken
};

__device__ __forceinline__ float dn_demod(float c, float a) { return c / fmaxf(a, 1e-3f); }

// (x, luminance) of pixel q as level i reads it: level 0 computes x0 = (colour / samples) / max(albedo, 1e-3) on the fly
template <bool FIRST>
__device__ __forceinline__ float4 dn_x(const DnLevel& L, size_t q) {
    if (FIRST) {
        const float4 c = L.color[q], a = L.ad[q];
        const float r = dn_demod(c.x / L.samples, a.x), g = dn_demod(c.y / L.samples, a.y), b = dn_demod(c.z / L.samples, a.z);
        return make_float4(r, g, b, dn_lum(r, g, b));
    }
    return L.xin[q];
}

// 5 x 5 taps q = p + s (dx, dy), dy outer, dx inner, both from -2 to 2.  Weight of a tap: (h[dx] * h[dy]) * ((wn * wz) * wl); the
// centre's is h[0]^2 exactly.  Taps outside the image or of class != 0 are skipped.  x_{i+1} = (sum of weight * x) / (sum of weight).
// LDS: the tile and its 2s halo are staged (out-of-image pixels as skipped taps); otherwise every tap is a global load (L2 / MALL).
template <bool LDS, bool FIRST, bool LAST>
__global__ __launch_bounds__(256) void k_dn_level(DnLevel L) {
    extern __shared__ float4 dn_lds[];   // [T*T] (x, l) then [T*T] guide, T = 16 + 4s
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
                if (g.w >= 0.0f) x = dn_x<FIRST>(L, q);
            }
            dn_lds[k] = x;
            dn_lds[T * T + k] = g;
        }
        __syncthreads();
    }
    if (px >= W || py >= H) return;
    const size_t p = (size_t)py * W + px;
    const int cp = LDS ? (ly + 2 * s) * T + (lx + 2 * s) : 0;
    const float4 gp = LDS ? dn_lds[T * T + cp] : L.guide[p];
    if (gp.w < 0.0f) {   // emissive or sky: returned unchanged, never filtered
        if (LAST) {
            const float4 c = L.color[p];
            L.xout[p] = make_float4(c.x / L.samples, c.y / L.samples, c.z / L.samples, c.w / L.samples);
        }
        return;
    }
    const float4 xp = LDS ? dn_lds[cp] : dn_x<FIRST>(L, p);
    const float hk[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    const float den_z = (L.sigma_z * gp.w) * (float)s;
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sw = 0.0f;
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = py + s * dy;
        if (!LDS && (qy < 0 || qy >= H)) continue;
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = px + s * dx;
            float4 gq, xq;
            if (LDS) {
                const int cq = cp + s * (dy * T + dx);
                gq = dn_lds[T * T + cq];
                if (gq.w < 0.0f) continue;
                xq = dn_lds[cq];
            } else {
                if (qx < 0 || qx >= W) continue;
                const size_t q = (size_t)qy * W + qx;
                gq = L.guide[q];
                if (gq.w < 0.0f) continue;
                xq = dn_x<FIRST>(L, q);
            }
            const float k = hk[dx + 2] * hk[dy + 2];
            float w;
            if (dx == 0 && dy == 0) {
                w = k;
            } else {
                const float nd = (gp.x * gq.x + gp.y * gq.y) + gp.z * gq.z;
                const float wn = powf(fmaxf(0.0f, nd), L.sigma_n);
                const float wz = expf(-fabsf(gp.w - gq.w) / den_z);
                const float wl = expf(-fabsf(xp.w - xq.w) / L.sigma_l);
                w = k * ((wn * wz) * wl);
            }
            sr = sr + w * xq.x;
            sg = sg + w * xq.y;
            sb = sb + w * xq.z;
            sw = sw + w;
        }
    }
    const float r = sr / sw, g = sg / sw, b = sb / sw;
    if (LAST) {
        const float4 a = L.ad[p], c = L.color[p];
        L.xout[p] = make_float4(r * fmaxf(a.x, 1e-3f), g * fmaxf(a.y, 1e-3f), b * fmaxf(a.z, 1e-3f), c.w / L.samples);
    } else {
        L.xout[p] = make_float4(r, g, b, dn_lum(r, g, b));
    }
}

template <bool LDS>
static const void* dn_level_kernel(bool first, bool last) {
    if (first) return last ? (const void*)k_dn_level<LDS, true, true> : (const void*)k_dn_level<LDS, true, false>;
    return last ? (const void*)k_dn_level<LDS, false, true> : (const void*)k_dn_level<LDS, false, false>;
}
