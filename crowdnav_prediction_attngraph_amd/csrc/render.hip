// render.hip -- rasteriser for batches of crowd scenes: cn_render_scenes draws the state of n envs into n RGBA8 images in ONE launch.
// It replaces the drawing half of the reference's render() (crowd_sim_pred.py:236-370, crowd_sim_var_num.py) for the vec-env slot
// render(mode='rgb_array') / get_images() (rl/vec_env/vec_env.py:121); the drawing rule is this project's own and is stated exactly in
// include/crowdnav_hip.h.  The translation unit does not see the simulator (EnvDev): every input is a caller-owned device buffer.
//
// Arithmetic: fp32, every operation rounded once (compiled with -ffp-contract=off), only + - *, comparisons and int -> float conversions in
// the per-pixel tests, so that a numpy float32 restatement reproduces every pixel (tests/render_ref.py).
//
// Kernel shape: a workgroup of 256 threads owns a 32 x 32 pixel tile of one env's image; a lane owns 4 horizontally adjacent pixels (8 lanes
// across, 32 rows) and writes them with one 16-byte store.  The env's shape list (ring, goal, dots, per human an outline and a heading mark,
// the robot's disc and mark) is staged in LDS 256 shapes at a time as pre-multiplied records, in paint order, after a cull against the tile:
// the cull evaluates the per-pixel expression itself at the tile's nearest (and, for a hole, farthest) pixel centre, and since every fp32
// operation involved is monotone in the pixel's coordinate, no pixel of the tile can pass a test that point fails -- conservative without an
// epsilon.  (The heading marks, whose test is not a distance, are culled by a disc that contains them with 1 % of slack.)
#include "common.h"

namespace {

constexpr int RN_TILE = 32;          // pixels per tile side
constexpr int RN_LX = RN_TILE / 4;   // lanes across a tile
constexpr int RN_THREADS = 256;      // = RN_LX * RN_TILE; also the shapes staged per round
constexpr int RN_MAX_DOTS = 1024;

enum { RN_ANNULUS = 0, RN_DIAMOND = 1, RN_MARK = 2 };

// 32 bytes, read by every lane of the workgroup at once (two broadcast ds_read_b128)
struct alignas(16) RnRec {
    float cx, cy;
    float a, b;        // annulus: lo^2 (-1: no hole), hi^2    diamond: radius, -    mark: vx, vy
    float c, d;        // mark: (r*r)*s2, (hw*hw)*s2
    uint32_t colour;
    int kind;
};

struct RnArgs {
    int n, H, max_dots, size, tiles_x, tiles;
    const double *humans, *robot;
    const int32_t *counts;
    const uint8_t *visible;
    const float *robot_heading, *dots;
    const int32_t *dot_counts;
    float robot_radius, ring_radius, q, L;
    uint32_t *out;
};

__host__ __device__ constexpr uint32_t rn_rgb(uint32_t r, uint32_t g, uint32_t b) { return r | (g << 8) | (b << 16) | (255u << 24); }
constexpr uint32_t RN_WHITE = rn_rgb(255, 255, 255), RN_GREY = rn_rgb(160, 160, 160), RN_GOAL = rn_rgb(220, 0, 0), RN_GREEN = rn_rgb(0, 160, 0),
                   RN_BLUE = rn_rgb(0, 0, 255), RN_RED = rn_rgb(255, 0, 0), RN_DARK = rn_rgb(160, 0, 0), RN_GOLD = rn_rgb(255, 215, 0);

__device__ __forceinline__ float rn_px(int j, float q, float L) { return ((float)j + 0.5f) * q - L; }
__device__ __forceinline__ float rn_py(int i, float q, float L) { return L - ((float)i + 0.5f) * q; }

// heading mark of a disc of radius r along v; false = no mark (s2 <= 1e-12)
__device__ __forceinline__ bool rn_mark(RnRec &rec, float cx, float cy, float r, float vx, float vy, float hw)
{
    const float s2 = vx * vx + vy * vy;
    rec.cx = cx; rec.cy = cy; rec.a = vx; rec.b = vy; rec.c = (r * r) * s2; rec.d = (hw * hw) * s2;
    rec.colour = RN_DARK; rec.kind = RN_MARK;
    return !(s2 <= 1e-12f);
}

__device__ __forceinline__ void rn_disc(RnRec &rec, float cx, float cy, float lo2, float hi2, uint32_t colour)
{
    rec.cx = cx; rec.cy = cy; rec.a = lo2; rec.b = hi2; rec.c = 0.0f; rec.d = 0.0f; rec.colour = colour; rec.kind = RN_ANNULUS;
}

__global__ __launch_bounds__(RN_THREADS) void render_scenes_kernel(RnArgs p)
{
    __shared__ RnRec recs[RN_THREADS];
    __shared__ int wave_cnt[RN_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int env = blockIdx.x / p.tiles, tile = blockIdx.x % p.tiles;
    const int S = p.size, H = p.H;
    const int col0 = (tile % p.tiles_x) * RN_TILE, row0 = (tile / p.tiles_x) * RN_TILE;
    const int col1 = min(col0 + RN_TILE, S) - 1, row1 = min(row0 + RN_TILE, S) - 1;
    const float q = p.q, L = p.L;
    const float w = 0.5f * q, hw = 0.75f * q, t = 1.5f * q;
    // the tile's outermost pixel centres
    const float xa = rn_px(col0, q, L), xb = rn_px(col1, q, L), yt = rn_py(row0, q, L), yb = rn_py(row1, q, L);

    const int col = col0 + (tid % RN_LX) * 4, row = row0 + tid / RN_LX;
    const float y = rn_py(row, q, L);
    float x[4];
    uint32_t pix[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { x[k] = rn_px(col + k, q, L); pix[k] = RN_WHITE; }

    int cnt = p.counts ? p.counts[env] : H;
    cnt = cnt < 0 ? 0 : (cnt > H ? H : cnt);
    int nd = 0;
    if (p.dots) {
        nd = p.dot_counts ? p.dot_counts[env] : p.max_dots;
        nd = nd < 0 ? 0 : (nd > p.max_dots ? p.max_dots : nd);
    }
    const double *rob = p.robot + (size_t)env * 8;
    const float rpx = (float)rob[0], rpy = (float)rob[1];
    // paint order: ring, goal, dots, (outline, mark) per human, robot disc, robot mark
    const int first_human = 2 + nd, first_robot = first_human + 2 * cnt, total = first_robot + 2;

    for (int base = 0; base < total; base += RN_THREADS) {
        const int k = base + tid;
        RnRec rec;
        bool keep = k < total;
        if (keep) {
            if (k == 0) {
                const float R = p.ring_radius, lo = R - w, hi = R + w;
                rn_disc(rec, rpx, rpy, lo * lo, hi * hi, RN_GREY);
                keep = R > 0.0f;
            } else if (k == 1) {
                rec.cx = (float)rob[4]; rec.cy = (float)rob[5]; rec.a = 0.3f; rec.b = 0.0f; rec.c = 0.0f; rec.d = 0.0f;
                rec.colour = RN_GOAL; rec.kind = RN_DIAMOND;
            } else if (k < first_human) {
                const float *dp = p.dots + ((size_t)env * p.max_dots + (k - 2)) * 2;
                rn_disc(rec, dp[0], dp[1], -1.0f, 0.12f * 0.12f, RN_GREEN);
            } else if (k < first_robot) {
                const int h = (k - first_human) >> 1;
                const double *hp = p.humans + ((size_t)env * H + h) * 8;
                const float cx = (float)hp[0], cy = (float)hp[1], r = (float)hp[6];
                if ((k - first_human) & 1) {
                    keep = rn_mark(rec, cx, cy, r, (float)hp[2], (float)hp[3], hw);
                } else {
                    const float ri = r - t;
                    const bool vis = p.visible ? p.visible[(size_t)env * H + h] != 0 : true;
                    rn_disc(rec, cx, cy, ri <= 0.0f ? -1.0f : ri * ri, r * r, vis ? RN_BLUE : RN_RED);
                }
            } else if (k == first_robot) {
                rn_disc(rec, rpx, rpy, -1.0f, p.robot_radius * p.robot_radius, RN_GOLD);
            } else {
                float vx, vy;
                if (p.robot_heading) { vx = p.robot_heading[(size_t)env * 2]; vy = p.robot_heading[(size_t)env * 2 + 1]; }
                else { vx = (float)rob[2]; vy = (float)rob[3]; }
                keep = rn_mark(rec, rpx, rpy, p.robot_radius, vx, vy, hw);
            }
        }
        if (keep) {
            // the per-pixel expressions at the tile's pixel centre nearest to the shape's centre: no pixel of the tile gets a smaller |dx|,
            // |dy|, d2 or |dx| + |dy| (x - cx, the squares and the sums are monotone in fp32 as they are in the reals)
            const float ndx = rec.cx < xa ? xa - rec.cx : (rec.cx > xb ? xb - rec.cx : 0.0f);
            const float ndy = rec.cy > yt ? yt - rec.cy : (rec.cy < yb ? yb - rec.cy : 0.0f);
            const float nd2 = ndx * ndx + ndy * ndy;
            if (rec.kind == RN_ANNULUS) {
                // ... and at the farthest one for the hole: no pixel gets a larger d2
                const float fdx = fmaxf(fabsf(xa - rec.cx), fabsf(xb - rec.cx)), fdy = fmaxf(fabsf(yt - rec.cy), fabsf(yb - rec.cy));
                const float fd2 = fdx * fdx + fdy * fdy;
                keep = !(nd2 > rec.b) && !(fd2 < rec.a);
            } else if (rec.kind == RN_DIAMOND) {
                keep = !(fabsf(ndx) + fabsf(ndy) > rec.a);
            } else {
                // a pixel on the mark has dot^2 <= (r*r)*s2 and cr^2 <= (hw*hw)*s2, and dot^2 + cr^2 = d2 * s2 but for rounding errors of a
                // relative 1e-6: 1 % of slack on the sum of the two bounds covers them many times over
                const float s2 = rec.a * rec.a + rec.b * rec.b;
                keep = !(nd2 * s2 > (rec.c + rec.d) * 1.01f);
            }
        }
        // ordered compaction: the kept shapes of this round, in list order
        const unsigned long long m = __ballot(keep);
        if (lane == 0) wave_cnt[wave] = __popcll(m);
        __syncthreads();
        int pos = __popcll(m & ((1ull << lane) - 1ull)), kept = 0;
#pragma unroll
        for (int v = 0; v < RN_THREADS / 64; ++v) {
            const int c = wave_cnt[v];
            pos += v < wave ? c : 0;
            kept += c;
        }
        if (keep) recs[pos] = rec;
        __syncthreads();

        for (int s = 0; s < kept; ++s) {
            const float4 A = reinterpret_cast<const float4 *>(&recs[s])[0];
            const float4 B = reinterpret_cast<const float4 *>(&recs[s])[1];
            const uint32_t colour = __float_as_uint(B.z);
            const int kind = __builtin_amdgcn_readfirstlane(__float_as_int(B.w)); // the same record in every lane
            const float dy = y - A.y;
            if (kind == RN_ANNULUS) {
                const float dy2 = dy * dy;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float dx = x[j] - A.x;
                    const float d2 = dx * dx + dy2;
                    if (d2 >= A.z && d2 <= A.w) pix[j] = colour;
                }
            } else if (kind == RN_DIAMOND) {
                const float ady = fabsf(dy);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float dx = x[j] - A.x;
                    if (fabsf(dx) + ady <= A.z) pix[j] = colour;
                }
            } else {
                const float vx = A.z, vy = A.w;
                const float dyvy = dy * vy, dyvx = dy * vx;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float dx = x[j] - A.x;
                    const float dot = dx * vx + dyvy, cr = dx * vy - dyvx;
                    if (dot >= 0.0f && dot * dot <= B.x && cr * cr <= B.y) pix[j] = colour;
                }
            }
        }
        if (base + RN_THREADS < total) __syncthreads(); // the next round overwrites the records
    }
    if (col < S && row < S) {
        uint32_t *dst = p.out + (((size_t)env * S + row) * (size_t)S + col);
        *reinterpret_cast<uint4 *>(dst) = make_uint4(pix[0], pix[1], pix[2], pix[3]);
    }
}

} // namespace

extern "C" int cn_render_scenes(int n, int H, const double *humans, const double *robot, const int32_t *counts, const uint8_t *visible,
                                const float *robot_heading, const float *dots, const int32_t *dot_counts, int max_dots, float robot_radius,
                                float ring_radius, int size, float half_width, uint32_t *out, void *stream)
{
    CN_REQUIRE(n >= 1, "cn_render_scenes: n=%d scenes (at least 1)", n);
    CN_REQUIRE(H >= 1 && H <= CN_MAX_HUMANS, "cn_render_scenes: H=%d human slots outside [1,%d]", H, CN_MAX_HUMANS);
    CN_REQUIRE(size >= 16 && size <= 1024 && size % 4 == 0, "cn_render_scenes: size=%d must be a multiple of 4 in [16,1024]", size);
    CN_REQUIRE(half_width > 0.0f, "cn_render_scenes: half_width must be positive");
    CN_REQUIRE(humans && robot && out, "cn_render_scenes: humans, robot and out are required");
    CN_REQUIRE(((uintptr_t)out & 15u) == 0, "cn_render_scenes: out must be 16-byte aligned");
    CN_REQUIRE(max_dots >= 0 && max_dots <= RN_MAX_DOTS, "cn_render_scenes: max_dots=%d outside [0,%d]", max_dots, RN_MAX_DOTS);
    CN_REQUIRE(!dots || max_dots >= 1, "cn_render_scenes: dots given with max_dots=%d", max_dots);
    RnArgs p;
    p.n = n; p.H = H; p.max_dots = max_dots; p.size = size;
    p.tiles_x = (size + RN_TILE - 1) / RN_TILE;
    p.tiles = p.tiles_x * p.tiles_x;
    CN_REQUIRE((long long)n * p.tiles < (1LL << 24), "cn_render_scenes: n=%d scenes of %d tiles each exceed one launch (2^24 workgroups)", n, p.tiles);
    p.humans = humans; p.robot = robot; p.counts = counts; p.visible = visible; p.robot_heading = robot_heading;
    p.dots = dots; p.dot_counts = dot_counts;
    p.robot_radius = robot_radius; p.ring_radius = ring_radius;
    p.q = (2.0f * half_width) / (float)size; // the pixel pitch, rounded once
    p.L = half_width;
    p.out = out;
    hipLaunchKernelGGL(render_scenes_kernel, dim3((unsigned)(n * p.tiles)), dim3(RN_THREADS), 0, (hipStream_t)stream, p);
    CN_CHECK_LAUNCH();
    return CN_OK;
}
