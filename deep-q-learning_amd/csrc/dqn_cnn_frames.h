// csrc/dqn_cnn_frames.h -- pixel envs for the CNN (included by dqn_cnn.hip): raw env images -> 84x84 luma -> four-frame stacks
// -> frame ring, one launch per vector env step (dqn_cnn_env_reset_frames / dqn_cnn_env_observe).
//
// The arithmetic (integer throughout, so the device output is bit-identical to a numpy restatement):
//   image X[F][H][W][C] u8, F in {1, 2}, C in {3, 1}, 84 <= H, W <= 512
//   Y = (4899 R + 9617 G + 1868 B + 8192) >> 14 (OpenCV's u8 luma weights; C = 1: Y = X)
//   M[y][x] = max_f Y_f[y][x]                                        (the frame-skip flicker fix; gray -> max -> resize)
//   area resize in units of 1/84 source pixel: source row r covers [84 r, 84 r + 84), output row i covers [H i, H i + H),
//   wr(i, r) = max(0, min(84 (r + 1), H (i + 1)) - max(84 r, H i)), wc(j, c) the same with W,
//   S = sum_r sum_c wr wc M[r][c] (<= 255 H W: int32), out[i][j] = (2 S + H W) / (2 H W) (the exact mean, rounded half up)
// Stacks are the CNN's NHWC [84][84][4] u8, one u32 per pixel, byte k = channel k, channel 3 the newest frame.
//
// Shape: one workgroup per (env, band of FRM_BAND output rows). It stages the band's source rows of all F frames in LDS with
// 16-byte loads (per-image offsets need not be 16-byte aligned: the pieces that straddle the span's ends are assembled from
// byte loads, nothing outside the span is read), reduces them to M (u8, LDS), then each thread resizes output pixels from M and
// moves whole u32 stack pixels: one read of the current stack, the ring's s and s' rows and the next current stack written.
#pragma once

constexpr int FRM_BAND = 6;                      // output rows per workgroup: 14 bands per image
constexpr int FRM_BANDS = 84 / FRM_BAND;
constexpr int FRM_PX = FRM_BAND * 84;            // 504 output pixels per band, two per thread
constexpr int FRM_STAGE = 16384;                 // raw bytes staged per pass: four 16-byte pieces per thread
constexpr int FRM_MROWS = 40;                    // source rows of a band: <= 6 H / 84 + 2 = 38 at H = 512
constexpr int FRM_MAX_HW = 512;
constexpr int STACK_PX = 84 * 84;

struct FrmGeo { int F, H, W, C; long long img; };     // img = F H W C bytes per env image

__device__ __forceinline__ uint32_t frm_luma(uint32_t r, uint32_t g, uint32_t b) { return (4899u * r + 9617u * g + 1868u * b + 8192u) >> 14; }

// the band starting at output row i0 of one image: out[u] = output pixel tid + 256 u of the band (u = 1 only for tid < 248)
__device__ void frm_band(const uint8_t *__restrict__ img, const FrmGeo &g, int i0, uint8_t *stg, uint8_t *mb, uint32_t (&out)[2]) {
    const int tid = threadIdx.x, H = g.H, W = g.W, C = g.C, F = g.F, rowb = W * C;
    const int r_lo = (H * i0) / 84, r_hi = (H * (i0 + FRM_BAND) + 83) / 84;
    const int half = FRM_STAGE / F;                                   // LDS bytes per frame in one pass (a multiple of 16)
    const int rows_per = (half - 16) / rowb;                          // >= 5 at W C = 1536, F = 2
    __syncthreads();                                                  // (stg / mb of the previous image are read out)
    for (int c0 = r_lo; c0 < r_hi; c0 += rows_per) {
        const int c1 = min(c0 + rows_per, r_hi), len = (c1 - c0) * rowb;
        // stage frame f's bytes [g0, g0 + len) at stg[f half + (g0 & 15) ...]: 16-byte pieces from the aligned address below g0
        uint4 v[4] = {};
        const int per_f = half / 16;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = tid + 256 * u, f = k / per_f, kk = k - f * per_f;
            if (f < F) {
                const uint8_t *g0 = img + ((long long)f * H + c0) * rowb;
                const int head = (int)((uintptr_t)g0 & 15);
                const uint8_t *p = g0 - head + 16 * kk;
                if (16 * kk < head + len) {
                    if (16 * kk >= head && 16 * kk + 16 <= head + len) v[u] = *reinterpret_cast<const uint4 *>(p);
                    else {
                        uint32_t w[4] = {0, 0, 0, 0};
                        for (int b = 0; b < 16; ++b) {
                            const int o = 16 * kk + b;
                            if (o >= head && o < head + len) w[b >> 2] |= (uint32_t)p[b] << (8 * (b & 3));
                        }
                        v[u] = uint4{w[0], w[1], w[2], w[3]};
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = tid + 256 * u, f = k / per_f, kk = k - f * per_f;
            if (f < F) {
                const int head = (int)((uintptr_t)(img + ((long long)f * H + c0) * rowb) & 15);
                if (16 * kk < head + len) *reinterpret_cast<uint4 *>(stg + f * half + 16 * kk) = v[u];
            }
        }
        __syncthreads();
        const int npx = (c1 - c0) * W;
        const int h0 = (int)((uintptr_t)(img + (long long)c0 * rowb) & 15);
        const int h1 = F > 1 ? (int)((uintptr_t)(img + ((long long)H + c0) * rowb) & 15) : 0;
        for (int p = tid; p < npx; p += 256) {
            const int row = p / W, x = p - row * W, o = row * rowb + x * C;
            const uint8_t *a = stg + h0 + o;
            uint32_t y = C == 3 ? frm_luma(a[0], a[1], a[2]) : a[0];
            if (F > 1) {
                const uint8_t *b = stg + half + h1 + o;
                const uint32_t y1 = C == 3 ? frm_luma(b[0], b[1], b[2]) : b[0];
                y = y1 > y ? y1 : y;
            }
            mb[(c0 - r_lo + row) * W + x] = (uint8_t)y;
        }
        __syncthreads();
    }
    const int HW2 = 2 * H * W;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int p = tid + 256 * u;
        if (p >= FRM_PX) break;
        const int i = i0 + p / 84, j = p % 84;
        const int rs = (H * i) / 84, re = (H * (i + 1) + 83) / 84, cs = (W * j) / 84, ce = (W * (j + 1) + 83) / 84;
        int S = 0;
        for (int r = rs; r < re; ++r) {
            const int wr = max(0, min(84 * (r + 1), H * (i + 1)) - max(84 * r, H * i));
            const uint8_t *mrow = mb + (r - r_lo) * W;
            int t = 0;
            for (int c = cs; c < ce; ++c) t += max(0, min(84 * (c + 1), W * (j + 1)) - max(84 * c, W * j)) * (int)mrow[c];
            S += wr * t;
        }
        out[u] = (uint32_t)((2 * S + H * W) / HW2);
    }
}

// INIT (dqn_cnn_env_reset_frames): cur[env] = the preprocessed raw[env] in all four channels (gym FrameStack.reset).
// Otherwise (dqn_cnn_env_observe), for env e at ring row pos + e:
//   s = cur[e]; s' = (s >> 8) | (out << 24); a, r, d as given;
//   cur[e] = reset_slot[e] in [0, m) ? the preprocessed reset_raw[reset_slot[e]] in all four channels : s'
__global__ void __launch_bounds__(256)
k_cnn_frames_init(const uint8_t *__restrict__ raw, FrmGeo g, uint32_t *__restrict__ cur) {
    __shared__ __attribute__((aligned(16))) uint8_t stg[FRM_STAGE];
    __shared__ uint8_t mb[FRM_MROWS * FRM_MAX_HW];
    const int band = blockIdx.x, env = blockIdx.y;
    uint32_t out[2];
    frm_band(raw + (long long)env * g.img, g, band * FRM_BAND, stg, mb, out);
    uint32_t *c = cur + (long long)env * STACK_PX + band * FRM_PX;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int p = threadIdx.x + 256 * u;
        if (p < FRM_PX) c[p] = out[u] * 0x01010101u;
    }
}

__global__ void __launch_bounds__(256)
k_cnn_frames_observe(const uint8_t *__restrict__ raw, const uint8_t *__restrict__ reset_raw, const int32_t *__restrict__ reset_slot, int m, FrmGeo g,
                     const int32_t *__restrict__ actions, const float *__restrict__ rewards, const float *__restrict__ dones,
                     uint32_t *__restrict__ cur, uint32_t *__restrict__ ring_s, uint32_t *__restrict__ ring_s2, int32_t *__restrict__ ring_a,
                     float *__restrict__ ring_r, float *__restrict__ ring_d, long long pos) {
    __shared__ __attribute__((aligned(16))) uint8_t stg[FRM_STAGE];
    __shared__ uint8_t mb[FRM_MROWS * FRM_MAX_HW];
    const int band = blockIdx.x, env = blockIdx.y, tid = threadIdx.x;
    uint32_t out[2], rout[2] = {0, 0};
    frm_band(raw + (long long)env * g.img, g, band * FRM_BAND, stg, mb, out);
    const int slot = reset_slot ? reset_slot[env] : -1;
    const bool reset = slot >= 0 && slot < m;                         // (anything else counts as -1)
    if (reset) frm_band(reset_raw + (long long)slot * g.img, g, band * FRM_BAND, stg, mb, rout);
    const long long px0 = band * FRM_PX;
    uint32_t *c = cur + (long long)env * STACK_PX + px0;
    uint32_t *s = ring_s + (pos + env) * STACK_PX + px0, *s2 = ring_s2 + (pos + env) * STACK_PX + px0;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int p = tid + 256 * u;
        if (p < FRM_PX) {
            const uint32_t v = c[p], nx = (v >> 8) | (out[u] << 24);
            s[p] = v; s2[p] = nx;
            c[p] = reset ? rout[u] * 0x01010101u : nx;
        }
    }
    if (band == 0 && tid == 0) { ring_a[pos + env] = actions[env]; ring_r[pos + env] = rewards[env]; ring_d[pos + env] = dones[env]; }
}
