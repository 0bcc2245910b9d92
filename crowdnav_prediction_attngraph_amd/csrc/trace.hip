// trace.hip -- what a recorded episode (cn_env_trace_append, env_sim.hip) is for: cn_trace_metrics measures n traces, cn_render_trajectories
// draws each of them as ONE picture.  Together they stand in for the per-episode trajectory figure the reference announces and never
// delivers (test.py:31 --render_traj, rl/networks/envs.py:226 VecPyTorch.render_traj -> env.render_traj, which no env class defines); both
// rules are this project's own and are stated exactly in include/crowdnav_hip.h.  The translation unit does not see the simulator: every
// input is a caller-owned device buffer in the trace layout (agents float32 [n,cap,A,6], flags uint8 [n,cap,A], length int32 [n]).
//
// Metrics: one wavefront per episode, lane h = human slot h; the records are walked in order, the robot's sums are plain sequential fp64
// sums over the records (every lane carries the same value), the per-human tests are combined by ballots and the minimum by a shuffle tree
// (a minimum does not depend on the order).  Compiled with -ffp-contract=off: a numpy loop in the same order gives the same bits.
//
// Figure: the kernel shape and the arithmetic rules of render.hip -- a workgroup of 256 threads per 32 x 32 tile, a lane owns 4 adjacent
// pixels and writes them with one 16-byte store; the episode's marks (up to cap * (2 H + 3): a trail disc and an outline per human and
// record, three marks per robot record) are generated 256 at a time in paint order, culled against the tile and staged in LDS.  Every mark
// is a disc or an annulus, so the cull is the one of render.hip: the per-pixel expression at the tile's nearest and, for a hole, farthest
// pixel centre; every fp32 operation involved is monotone in the pixel's coordinate, so no pixel of the tile can pass a test that point
// fails -- conservative without an epsilon.  The goal diamond is one shape per image: every lane tests it directly, before the rounds.
#include "common.h"

namespace {

constexpr int TR_TILE = 32;          // pixels per tile side
constexpr int TR_LX = TR_TILE / 4;   // lanes across a tile
constexpr int TR_THREADS = 256;      // = TR_LX * TR_TILE; also the marks generated per round
constexpr int TR_MAX_CAP = 1 << 16;  // records per episode

// ---------------------------------------------------------------- metrics ----------------------------------------------------------------
__global__ __launch_bounds__(64) void trace_metrics_kernel(int cap, int A, const float *agents, const uint8_t *flags, const int32_t *length,
                                                           double time_step, double discomfort_dist, double *out)
{
    const int e = blockIdx.x, lane = threadIdx.x;
    int L = length[e];
    L = L < 0 ? 0 : (L > cap ? cap : L);
    const bool slot = lane < A - 1;
    double path = 0.0, speed = 0.0, accel = 0.0, clear = INFINITY;
    double ppx = 0.0, ppy = 0.0, pvx = 0.0, pvy = 0.0;
    long long intr = 0, vis_intr = 0, crowd = 0;
    for (int t = 0; t < L; ++t) {
        const size_t rec = ((size_t)e * cap + t) * A;
        const float *rp = agents + rec * 6;
        const double px = (double)rp[0], py = (double)rp[1], vx = (double)rp[2], vy = (double)rp[3], rr = (double)rp[4];
        speed += sqrt(vx * vx + vy * vy);
        if (t > 0) {
            const double dx = px - ppx, dy = py - ppy, ax = vx - pvx, ay = vy - pvy;
            path += sqrt(dx * dx + dy * dy);
            accel += sqrt(ax * ax + ay * ay);
        }
        ppx = px; ppy = py; pvx = vx; pvy = vy;
        bool present = false, close = false, vclose = false;
        if (slot) {
            const uint8_t fl = flags[rec + 1 + lane];
            present = (fl & 1) != 0;
            if (present) {
                const float *hp = rp + (size_t)(1 + lane) * 6;
                const double dx = px - (double)hp[0], dy = py - (double)hp[1];
                const double c = sqrt(dx * dx + dy * dy) - rr - (double)hp[4];
                clear = c < clear ? c : clear;
                close = c < discomfort_dist;
                vclose = close && (fl & 2) != 0;
            }
        }
        crowd += __popcll(__ballot(present));
        intr += __ballot(close) != 0 ? 1 : 0;
        vis_intr += __ballot(vclose) != 0 ? 1 : 0;
    }
    for (int off = 32; off >= 1; off >>= 1) {
        const double o = __shfl_xor(clear, off, 64);
        clear = o < clear ? o : clear;
    }
    if (lane == 0) {
        double *o = out + (size_t)e * CN_TRACE_METRICS;
        o[CN_TRACE_RECORDS] = (double)L;
        o[CN_TRACE_PATH_LENGTH] = path;
        o[CN_TRACE_MIN_CLEARANCE] = clear;
        o[CN_TRACE_INTRUSION_STEPS] = (double)intr;
        o[CN_TRACE_VISIBLE_INTRUSION_STEPS] = (double)vis_intr;
        o[CN_TRACE_MEAN_SPEED] = L > 0 ? speed / (double)L : 0.0;
        o[CN_TRACE_MEAN_ACCEL] = L > 1 ? accel / ((double)(L - 1) * time_step) : 0.0;
        o[CN_TRACE_MEAN_CROWD] = L > 0 ? (double)crowd / (double)L : 0.0;
    }
}

// ---------------------------------------------------------------- figure -----------------------------------------------------------------
// 32 bytes, read by every lane of the workgroup at once (two broadcast ds_read_b128)
struct alignas(16) TrRec {
    float cx, cy;
    float lo2, hi2;    // d2 >= lo2 (-1: no hole) && d2 <= hi2
    uint32_t colour;
    uint32_t pad[3];
};

struct TrArgs {
    int n, cap, A, stride, size, tiles_x, tiles;
    const float *agents;
    const uint8_t *flags;
    const int32_t *length;
    const float *goal;
    float q, L;
    uint32_t *out;
};

__device__ __forceinline__ uint32_t tr_rgb(uint32_t r, uint32_t g, uint32_t b) { return r | (g << 8) | (b << 16) | (255u << 24); }
__device__ __forceinline__ float tr_px(int j, float q, float L) { return ((float)j + 0.5f) * q - L; }
__device__ __forceinline__ float tr_py(int i, float q, float L) { return L - ((float)i + 0.5f) * q; }

__global__ __launch_bounds__(TR_THREADS) void render_trajectories_kernel(TrArgs p)
{
    __shared__ TrRec recs[TR_THREADS];
    __shared__ int wave_cnt[TR_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ep = blockIdx.x / p.tiles, tile = blockIdx.x % p.tiles;
    const int S = p.size, A = p.A, H = A - 1, cap = p.cap, stride = p.stride;
    const int col0 = (tile % p.tiles_x) * TR_TILE, row0 = (tile / p.tiles_x) * TR_TILE;
    const int col1 = min(col0 + TR_TILE, S) - 1, row1 = min(row0 + TR_TILE, S) - 1;
    const float q = p.q, Lw = p.L;
    const float th = 1.5f * q;
    // the tile's outermost pixel centres
    const float xa = tr_px(col0, q, Lw), xb = tr_px(col1, q, Lw), yt = tr_py(row0, q, Lw), yb = tr_py(row1, q, Lw);

    const int col = col0 + (tid % TR_LX) * 4, row = row0 + tid / TR_LX;
    const float y = tr_py(row, q, Lw);
    float x[4];
    uint32_t pix[4];
    {   // layers 0 and 1: white, the goal diamond
        const float gx = p.goal[(size_t)ep * 2], gy = p.goal[(size_t)ep * 2 + 1];
        const float ady = fabsf(y - gy);
        const uint32_t white = tr_rgb(255, 255, 255), red = tr_rgb(220, 0, 0);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            x[k] = tr_px(col + k, q, Lw);
            pix[k] = fabsf(x[k] - gx) + ady <= 0.3f ? red : white;
        }
    }

    int L = p.length[ep];
    L = L < 0 ? 0 : (L > cap ? cap : L);
    const int D = L - 1 > 1 ? L - 1 : 1;
    const float *ag = p.agents + (size_t)ep * cap * A * 6;
    const uint8_t *fg = p.flags + (size_t)ep * cap * A;
    // paint order: per record and human slot (trail disc, outline), then per record of the robot (trail disc, outline, full disc)
    const int first_robot = L * H * 2, total = first_robot + L * 3;

    for (int base = 0; base < total; base += TR_THREADS) {
        const int k = base + tid;
        TrRec rec;
        bool keep = k < total;
        if (keep) {
            int t, a, sub;
            if (k < first_robot) { const int m = k >> 1; sub = k & 1; t = m / H; a = 1 + (m - t * H); }
            else { const int m = k - first_robot; t = m / 3; sub = m - t * 3; a = 0; }
            const size_t slot = (size_t)t * A + a;
            const uint8_t fl = a ? fg[slot] : (uint8_t)1;
            const bool last = t == L - 1;
            const bool stamp = last || t % stride == 0;
            keep = (fl & 1) != 0 && (sub == 0 || (sub == 1 ? stamp : last));
            if (keep) {
                const float *r = ag + slot * 6;
                const float rad = r[4];
                const uint32_t s = (uint32_t)((t * 160) / D);
                rec.cx = r[0]; rec.cy = r[1];
                rec.colour = a == 0 ? tr_rgb(255, 215 - s, 0) : ((fl & 2) ? tr_rgb(200 - s, 200 - s, 255) : tr_rgb(255, 200 - s, 200 - s));
                rec.pad[0] = rec.pad[1] = rec.pad[2] = 0;
                if (sub == 0) { const float rt = 0.4f * rad; rec.lo2 = -1.0f; rec.hi2 = rt * rt; }
                else if (sub == 1) { const float ri = rad - th; rec.lo2 = ri <= 0.0f ? -1.0f : ri * ri; rec.hi2 = rad * rad; }
                else { rec.lo2 = -1.0f; rec.hi2 = rad * rad; }
                // the per-pixel expression at the tile's pixel centre nearest to the mark's centre: no pixel of the tile gets a smaller d2
                // (x - cx, the squares and the sum are monotone in fp32 as they are in the reals) ...
                const float ndx = rec.cx < xa ? xa - rec.cx : (rec.cx > xb ? xb - rec.cx : 0.0f);
                const float ndy = rec.cy > yt ? yt - rec.cy : (rec.cy < yb ? yb - rec.cy : 0.0f);
                const float nd2 = ndx * ndx + ndy * ndy;
                // ... and at the farthest one for the hole: no pixel gets a larger d2
                const float fdx = fmaxf(fabsf(xa - rec.cx), fabsf(xb - rec.cx)), fdy = fmaxf(fabsf(yt - rec.cy), fabsf(yb - rec.cy));
                const float fd2 = fdx * fdx + fdy * fdy;
                keep = !(nd2 > rec.hi2) && !(fd2 < rec.lo2);
            }
        }
        // ordered compaction: the kept marks of this round, in list order
        const unsigned long long m = __ballot(keep);
        if (lane == 0) wave_cnt[wave] = __popcll(m);
        __syncthreads();
        int pos = __popcll(m & ((1ull << lane) - 1ull)), kept = 0;
#pragma unroll
        for (int v = 0; v < TR_THREADS / 64; ++v) {
            const int c = wave_cnt[v];
            pos += v < wave ? c : 0;
            kept += c;
        }
        if (keep) recs[pos] = rec;
        __syncthreads();

        for (int s = 0; s < kept; ++s) {
            const float4 R = reinterpret_cast<const float4 *>(&recs[s])[0];
            const uint32_t colour = recs[s].colour;
            const float dy = y - R.y;
            const float dy2 = dy * dy;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float dx = x[j] - R.x;
                const float d2 = dx * dx + dy2;
                if (d2 >= R.z && d2 <= R.w) pix[j] = colour;
            }
        }
        if (base + TR_THREADS < total) __syncthreads(); // the next round overwrites the records (and wave_cnt)
    }
    if (col < S && row < S) {
        uint32_t *dst = p.out + (((size_t)ep * S + row) * (size_t)S + col);
        *reinterpret_cast<uint4 *>(dst) = make_uint4(pix[0], pix[1], pix[2], pix[3]);
    }
}

int check_trace(const char *who, int n, int cap, int A, const float *agents, const uint8_t *flags, const int32_t *length)
{
    CN_REQUIRE(n >= 1, "%s: n=%d episodes (at least 1)", who, n);
    CN_REQUIRE(cap >= 1 && cap <= TR_MAX_CAP, "%s: cap=%d records per episode outside [1,%d]", who, cap, TR_MAX_CAP);
    CN_REQUIRE(A >= 2 && A <= CN_MAX_HUMANS + 1, "%s: A=%d agent slots outside [2,%d]", who, A, CN_MAX_HUMANS + 1);
    CN_REQUIRE(agents && flags && length, "%s: agents, flags and length are required", who);
    return CN_OK;
}

} // namespace

extern "C" int cn_trace_metrics(int n, int cap, int A, const float *agents, const uint8_t *flags, const int32_t *length, double time_step,
                                double discomfort_dist, double *out, void *stream)
{
    if (int rc = check_trace("cn_trace_metrics", n, cap, A, agents, flags, length)) return rc;
    CN_REQUIRE(out, "cn_trace_metrics: out is required");
    CN_REQUIRE(time_step > 0.0, "cn_trace_metrics: time_step must be positive");
    hipLaunchKernelGGL(trace_metrics_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, cap, A, agents, flags, length, time_step,
                       discomfort_dist, out);
    CN_CHECK_LAUNCH();
    return CN_OK;
}

extern "C" int cn_render_trajectories(int n, int cap, int A, const float *agents, const uint8_t *flags, const int32_t *length, const float *goal,
                                      int stride, int size, float half_width, uint32_t *out, void *stream)
{
    if (int rc = check_trace("cn_render_trajectories", n, cap, A, agents, flags, length)) return rc;
    CN_REQUIRE(goal && out, "cn_render_trajectories: goal and out are required");
    CN_REQUIRE(stride >= 1, "cn_render_trajectories: stride=%d (at least 1)", stride);
    CN_REQUIRE(size >= 16 && size <= 1024 && size % 4 == 0, "cn_render_trajectories: size=%d must be a multiple of 4 in [16,1024]", size);
    CN_REQUIRE(half_width > 0.0f, "cn_render_trajectories: half_width must be positive");
    CN_REQUIRE(((uintptr_t)out & 15u) == 0, "cn_render_trajectories: out must be 16-byte aligned");
    TrArgs p;
    p.n = n; p.cap = cap; p.A = A; p.stride = stride; p.size = size;
    p.tiles_x = (size + TR_TILE - 1) / TR_TILE;
    p.tiles = p.tiles_x * p.tiles_x;
    CN_REQUIRE((long long)n * p.tiles < (1LL << 24), "cn_render_trajectories: n=%d episodes of %d tiles each exceed one launch (2^24 workgroups)", n,
               p.tiles);
    p.agents = agents; p.flags = flags; p.length = length; p.goal = goal;
    p.q = (2.0f * half_width) / (float)size; // the pixel pitch, rounded once
    p.L = half_width;
    p.out = out;
    hipLaunchKernelGGL(render_trajectories_kernel, dim3((unsigned)(n * p.tiles)), dim3(TR_THREADS), 0, (hipStream_t)stream, p);
    CN_CHECK_LAUNCH();
    return CN_OK;
}
