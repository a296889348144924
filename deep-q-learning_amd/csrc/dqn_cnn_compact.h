// csrc/dqn_cnn_compact.h -- the compact frame ring (dqn_cnn_replay_init_compact; included by dqn_cnn.hip after k_cnn_gather):
// every preprocessed 84x84 frame stored once, the four-frame stacks put together at sample time. DESIGN.md 4.4f.
//
// Layout. A frame plane of C_f = capacity + 4 max_batch slots of 7056 bytes; ring row with global counter c (position c mod
// capacity) owns slot c mod C_f, which holds the NEWEST frame of its s. Per row, besides a / r / d, one meta word:
// slot | k << 30, k = the row's step within its episode clamped to 3. With n = the env count (rows are step-major, n per vector step),
// f(x) = the plane at slot x mod C_f:
//   s(p)[c]  = f(slot(p) - min(3 - c, k(p)) n)
//   s'(p)[c] = f(slot(p) - min(2 - c, k(p)) n)   c < 3
//   s'(p)[3] = f(slot(p) + n)                      (written by the observe that filed row p: the next frame of its env)
// min(., k) repeats an episode's first frame, as gym FrameStack after a reset (and the full ring's stacks). The one difference
// from the full ring: a row whose env was reset stores no terminal frame, so its s'[3] is the next episode's first frame. Such rows
// carry d = 1, and both TD rules multiply that term by (1 - d) = 0.
// Lifetime: with the ring full, the oldest live row reads 3 steps (3 n slots) behind it and the newest observe wrote n slots
// ahead of the head, so live rows reference capacity + 4 n <= C_f consecutive slots: none is overwritten while a row needs it.
#pragma once

constexpr int CMP_K_SHIFT = 30;                        // meta word = slot | k << 30 (slot < 2^24 + 2^18)
constexpr uint32_t CMP_SLOT_MASK = (1u << CMP_K_SHIFT) - 1;
constexpr int CMP_GROUPS = STACK_PX / 16;              // 441 groups of 16 pixels per frame (16-byte loads of a plane)
constexpr int CMP_GROUPS_PER_WG = (CMP_GROUPS + 1) / 2;

__device__ __forceinline__ long long cmp_slot(long long x, long long cf) { x %= cf; return x < 0 ? x + cf : x; }
// x mod cf for -cf <= x < 2 cf (slots are below 2^25: 32-bit arithmetic, no division)
__device__ __forceinline__ int cmp_wrap(int x, int cf) { return x < 0 ? x + cf : (x >= cf ? x - cf : x); }

// the compact ring's side of dqn_cnn_env_reset_frames (behind k_cnn_frames_init): env e's first frame (channel 3 of its stack)
// into slot (ctr + e) mod C_f, k_env[e] = 0. One workgroup per env, one u32 of the plane (4 pixels) per thread step.
__global__ void __launch_bounds__(256)
k_cnn_compact_seed(const uint32_t *__restrict__ cur, uint8_t *__restrict__ plane, long long cf, long long ctr, int32_t *__restrict__ k_env) {
    const int env = blockIdx.x;
    const uint4 *src = reinterpret_cast<const uint4 *>(cur + (long long)env * STACK_PX);
    uint32_t *dst = reinterpret_cast<uint32_t *>(plane + cmp_slot(ctr + env, cf) * STACK_PX);
    for (int p = threadIdx.x; p < STACK_PX / 4; p += 256) {
        const uint4 v = src[p];
        dst[p] = (v.x >> 24) | ((v.y >> 24) << 8) | ((v.z >> 24) << 16) | (v.w & 0xff000000u);
    }
    if (threadIdx.x == 0) k_env[env] = 0;
}

// dqn_cnn_env_observe on a compact ring: the preprocessing of k_cnn_frames_observe (frm_band, the same bits) and the same update
// of the envs' current stacks (env_act reads them), but instead of two whole stacks per row it files
//   plane slot (ctr + n + e) mod C_f = the env's next frame: the reset image when reset_slot[e] is in [0, m), else the step image,
//   a, r, d and meta = slot (ctr + e) mod C_f | k_env[e] << 30 at row pos + e; k_env[e] = reset ? 0 : min(k_env[e] + 1, 3).
// The band's 504 bytes go through LDS to 63 eight-byte stores (slot bases are 16-byte aligned, band offsets 8-byte aligned).
__global__ void __launch_bounds__(256)
k_cnn_compact_observe(const uint8_t *__restrict__ raw, const uint8_t *__restrict__ reset_raw, const int32_t *__restrict__ reset_slot, int m, FrmGeo g,
                      const int32_t *__restrict__ actions, const float *__restrict__ rewards, const float *__restrict__ dones,
                      uint32_t *__restrict__ cur, int32_t *__restrict__ k_env, uint8_t *__restrict__ plane, long long cf, int32_t *__restrict__ ring_a,
                      float *__restrict__ ring_r, float *__restrict__ ring_d, uint32_t *__restrict__ ring_meta, long long pos, long long ctr, int n) {
    __shared__ __attribute__((aligned(16))) uint8_t stg[FRM_STAGE];
    __shared__ uint8_t mb[FRM_MROWS * FRM_MAX_HW];
    __shared__ __attribute__((aligned(16))) uint8_t nb[FRM_PX];
    const int band = blockIdx.x, env = blockIdx.y, tid = threadIdx.x;
    uint32_t out[2], rout[2] = {0, 0};
    frm_band(raw + (long long)env * g.img, g, band * FRM_BAND, stg, mb, out);
    const int slot = reset_slot ? reset_slot[env] : -1;
    const bool reset = slot >= 0 && slot < m;                         // (anything else counts as -1)
    if (reset) frm_band(reset_raw + (long long)slot * g.img, g, band * FRM_BAND, stg, mb, rout);
    uint32_t *c = cur + (long long)env * STACK_PX + band * FRM_PX;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int p = tid + 256 * u;
        if (p < FRM_PX) {
            const uint32_t nx = (c[p] >> 8) | (out[u] << 24);
            c[p] = reset ? rout[u] * 0x01010101u : nx;
            nb[p] = (uint8_t)(reset ? rout[u] : out[u]);
        }
    }
    __syncthreads();
    uint2 *dst = reinterpret_cast<uint2 *>(plane + cmp_slot(ctr + n + env, cf) * STACK_PX + band * FRM_PX);
    if (tid < FRM_PX / 8) dst[tid] = reinterpret_cast<const uint2 *>(nb)[tid];
    if (band == 0 && tid == 0) {
        const int k = k_env[env];
        ring_a[pos + env] = actions[env]; ring_r[pos + env] = rewards[env]; ring_d[pos + env] = dones[env];
        ring_meta[pos + env] = (uint32_t)cmp_slot(ctr + env, cf) | ((uint32_t)k << CMP_K_SHIFT);
        k_env[env] = reset ? 0 : (k < 3 ? k + 1 : 3);
    }
}

// four words of four pixels each (w[c] = channel c of pixels 0..3, byte j = pixel j) -> the four NHWC u32 pixels (byte c = channel c)
__device__ __forceinline__ uint4 cmp_interleave(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3) {
    const uint32_t lo01 = (w0 & 0x000000ffu) | ((w1 & 0x000000ffu) << 8) | ((w0 & 0x0000ff00u) << 8) | ((w1 & 0x0000ff00u) << 16);
    const uint32_t hi01 = ((w0 & 0x00ff0000u) >> 16) | ((w1 & 0x00ff0000u) >> 8) | ((w0 & 0xff000000u) >> 8) | (w1 & 0xff000000u);
    const uint32_t lo23 = (w2 & 0x000000ffu) | ((w3 & 0x000000ffu) << 8) | ((w2 & 0x0000ff00u) << 8) | ((w3 & 0x0000ff00u) << 16);
    const uint32_t hi23 = ((w2 & 0x00ff0000u) >> 16) | ((w3 & 0x00ff0000u) >> 8) | ((w2 & 0xff000000u) >> 8) | (w3 & 0xff000000u);
    return uint4{(lo01 & 0xffffu) | (lo23 << 16), (lo01 >> 16) | (lo23 & 0xffff0000u), (hi01 & 0xffffu) | (hi23 << 16), (hi01 >> 16) | (hi23 & 0xffff0000u)};
}
__device__ __forceinline__ void cmp_interleave16(const uint4 &a, const uint4 &b, const uint4 &c, const uint4 &d, uint4 *dst) {
    dst[0] = cmp_interleave(a.x, b.x, c.x, d.x); dst[1] = cmp_interleave(a.y, b.y, c.y, d.y);
    dst[2] = cmp_interleave(a.z, b.z, c.z, d.z); dst[3] = cmp_interleave(a.w, b.w, c.w, d.w);
}

// k_cnn_gather for the compact ring: workgroup (sample i, half q of the 441 sixteen-pixel groups). Each thread reads 16 pixels of
// the planes of s (4) and s' (4; for n_step = 1 the same row, so only s'[3] is new: 5 planes), interleaves them into 16 NHWC
// pixels of s and of s' (four 16-byte stores each). Row indices are clamped as in k_cnn_gather and every slot is taken mod C_f,
// so no index or meta word can lead outside the plane. The scalars are k_cnn_gather's (cnn_gather_scalars), the n-step s' is the
// last row's.
__global__ void __launch_bounds__(256)
k_cnn_compact_gather(const uint8_t *__restrict__ plane, int cf, const uint32_t *__restrict__ ring_meta, const int32_t *__restrict__ ring_a,
                     const float *__restrict__ ring_r, const float *__restrict__ ring_d, const int32_t *__restrict__ idx, int B, long long cap,
                     int n_step, int n_envs, int env_n, float gamma, uint8_t *__restrict__ s, uint8_t *__restrict__ s2, int32_t *__restrict__ a,
                     float *__restrict__ r, float *__restrict__ d) {
    const int i = blockIdx.x, q = blockIdx.y, tid = threadIdx.x;
    long long row = idx[i];
    row = row < 0 ? 0 : (row >= cap ? cap - 1 : row);
    const long long row_last = (row + (long long)(n_step - 1) * n_envs) % cap;
    const uint32_t m0 = ring_meta[row], m1 = ring_meta[row_last];
    // (the % only guards against a meta word no kernel wrote; 3 env_n <= 3 max_batch < C_f keeps every offset in cmp_wrap's range)
    const int sl0 = (int)((m0 & CMP_SLOT_MASK) % (uint32_t)cf), sl1 = (int)((m1 & CMP_SLOT_MASK) % (uint32_t)cf);
    const int k0 = (int)(m0 >> CMP_K_SHIFT), k1 = (int)(m1 >> CMP_K_SHIFT);
    auto at = [&](int slot) { return reinterpret_cast<const uint4 *>(plane + (long long)slot * STACK_PX); };
    const uint4 *f[8];
#pragma unroll
    for (int c = 0; c < 4; ++c) f[c] = at(cmp_wrap(sl0 - min(3 - c, k0) * env_n, cf));
#pragma unroll
    for (int c = 0; c < 3; ++c) f[4 + c] = at(cmp_wrap(sl1 - min(2 - c, k1) * env_n, cf));
    f[7] = at(cmp_wrap(sl1 + env_n, cf));
    const int gi = q * CMP_GROUPS_PER_WG + tid;
    if (tid < CMP_GROUPS_PER_WG && gi < CMP_GROUPS) {
        uint4 *ds = reinterpret_cast<uint4 *>(s + (long long)i * CNN_FRAME_BYTES) + 4 * gi, *d2 = reinterpret_cast<uint4 *>(s2 + (long long)i * CNN_FRAME_BYTES) + 4 * gi;
        const uint4 p0 = f[0][gi], p1 = f[1][gi], p2 = f[2][gi], p3 = f[3][gi], n3 = f[7][gi];
        cmp_interleave16(p0, p1, p2, p3, ds);
        if (row_last == row) cmp_interleave16(p1, p2, p3, n3, d2);   // s'[c] = s[c + 1] for c < 3
        else cmp_interleave16(f[4][gi], f[5][gi], f[6][gi], n3, d2);
    }
    if (q == 0 && tid == 0) cnn_gather_scalars(ring_a, ring_r, ring_d, row, cap, n_step, n_envs, gamma, i, a, r, d);
}
