// gst_data.hip -- the GST predictor's training data on the device: the (5 + P)-frame sequences of gst_updated/src/mgnn/trajectories.py
// (TrajectoriesDataset: obs 5, pred P = pred_seq_len in 1 .. CN_MAX_PRED, 5 through the entry points without a horizon; skip 1, frame_diff 1,
// invalid -999) cut out of the collect batch's observation log, and the minibatch
// assembly (seq_to_graph's vertices, rotate_graph, padding) that feeds cn_gst_train_step / cn_gst_eval_step.  The rule is stated in
// include/crowdnav_hip.h; the host class is its definition and tests/test_gpu_gst_data.py compares every output bit for bit.
//
// Arithmetic: compiled with -ffp-contract=off.  A displacement is the float64 difference of the two float32 positions rounded once to float32
// (what the host computes from the parsed text); a rotation is x*c - y*s, x*s + y*c in fp32 with every product and sum rounded once.
//
// Kernel shape: the output is ragged, so it is built in two passes around an exclusive sum the caller runs (count, then fill): no atomics on
// the data, no order that depends on timing.  One wavefront per (sample, env) classifies a sample; one wavefront per candidate window ranks the
// window's at most (5 + P) * H <= 13 * 64 = 832 prediction ids (GD_MAX_ROWS: every LDS array of a window holds that many) in LDS by counting (O(n^2) LDS broadcasts -- the pass runs once per dataset).  The only atomic
// is an OR into the status word, whose result does not depend on order.
#include "common.h"

namespace {

constexpr int GD_OBS = 5;                            // observed frames of a window; a window is T = GD_OBS + P frames (GdArgs::T)
constexpr int GD_TMAX = GD_OBS + CN_MAX_PRED;        // the longest window
constexpr int GD_MAX_ROWS = GD_TMAX * CN_MAX_HUMANS; // rows of the longest window
constexpr float GD_INVALID = -999.0f;

// visible = the row collect_data.py writes: its last column is not infinite (collect.format_rows)
__device__ __forceinline__ bool gd_visible(float py) { return !isinf(py); }

// ---- pass 0: one wavefront per (sample f, env e): is anybody visible, the sample's frame id, the per-sample refusals ----
__global__ __launch_bounds__(64) void gd_frames_kernel(int FE, int H, const float4 *__restrict__ log, int32_t *__restrict__ visible,
                                                       float *__restrict__ frame_id, int32_t *__restrict__ status)
{
    const int fe = blockIdx.x, lane = threadIdx.x;
    if (fe >= FE) return;
    float4 row = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    bool vis = false;
    if (lane < H) {
        row = log[(size_t)fe * H + lane];
        vis = gd_visible(row.w);
    }
    const uint64_t vmask = __ballot(vis);
    const int first = vmask ? __ffsll((unsigned long long)vmask) - 1 : 0;
    const float fid = __shfl(row.x, first, 64);
    bool bad_frame = vis && !(row.x == fid), dup = false;
    for (int m = 0; m < H; ++m) {
        const float idm = __shfl(row.y, m, 64);
        dup |= vis && ((vmask >> m) & 1ull) && m != lane && idm == row.y;
    }
    int bits = (__ballot(bad_frame) ? CN_GSTD_FRAME_ORDER : 0) | (__ballot(dup) ? CN_GSTD_DUPLICATE_ID : 0);
    if (lane == 0) {
        visible[fe] = vmask ? 1 : 0;
        frame_id[fe] = vmask ? fid : 0.0f;
        if (bits) atomicOr(status, bits);
    }
}

// ---- pass 1a: the listed samples of every env in order (listed_before = exclusive sum of `visible` along f) ----
__global__ void gd_compact_kernel(int F, int E, const int32_t *__restrict__ visible, const int32_t *__restrict__ listed_before,
                                  int32_t *__restrict__ frame_list)
{
    const int fe = blockIdx.x * blockDim.x + threadIdx.x;
    if (fe >= F * E) return;
    const int f = fe / E, e = fe - f * E;
    const int j = listed_before[fe];
    if (visible[fe] && j >= 0 && j < F) frame_list[(size_t)e * F + j] = f;
}

__device__ __forceinline__ int gd_listed(int F, int E, int e, const int32_t *visible, const int32_t *listed_before)
{
    const size_t last = (size_t)(F - 1) * E + e;
    const int n = listed_before[last] + (visible[last] ? 1 : 0);
    return n < 0 ? 0 : (n > F ? F : n);
}

// ---- pass 1b: frame ids strictly increase along every env's list ----
__global__ void gd_order_kernel(int F, int E, const int32_t *__restrict__ visible, const int32_t *__restrict__ listed_before,
                                const int32_t *__restrict__ frame_list, const float *__restrict__ frame_id, int32_t *__restrict__ status)
{
    const int ej = blockIdx.x * blockDim.x + threadIdx.x;
    if (ej >= E * F) return;
    const int e = ej / F, j = ej - e * F;
    if (j + 1 >= gd_listed(F, E, e, visible, listed_before)) return;
    const int f0 = frame_list[(size_t)e * F + j], f1 = frame_list[(size_t)e * F + j + 1];
    if (f0 < 0 || f0 >= F || f1 < 0 || f1 >= F) return;
    if (!(frame_id[(size_t)f1 * E + e] > frame_id[(size_t)f0 * E + e])) atomicOr(status, (int)CN_GSTD_FRAME_ORDER);
}

// One candidate window in LDS.  sid: prediction id of row j = k * H + h (NaN = not visible: it compares unequal to and not below anything);
// srank: the row's pedestrian slot = number of distinct ids below its own.
struct GdWindow {
    float sid[GD_MAX_ROWS];
    int16_t srank[GD_MAX_ROWS];
    uint8_t sfirst[GD_MAX_ROWS];
    int32_t frames[GD_TMAX];
};

struct GdArgs {
    int F, E, H, W, mode, T;   // T = GD_OBS + P frames per window, W = F - (T - 1) candidates per env
    const float *log;
    const int32_t *visible, *listed_before, *frame_list;
    const float *frame_id;
};

// Is candidate `cand` = e * W + i a window of this env in this mode?  Fills w.frames.  Uniform over the wavefront.
__device__ __forceinline__ bool gd_candidate(const GdArgs &p, int cand, GdWindow &w, int &e_out, float &fid0)
{
    const int e = cand / p.W, i = cand - e * p.W;
    e_out = e;
    const int nw = gd_listed(p.F, p.E, e, p.visible, p.listed_before) - (p.T - 1); // W of this env
    if (i >= nw) return false;
    // TrajectoriesDataset: stop = nw + 1; 'train' = range(0, int(stop * 0.8)), 'val' / 'test' = range(int(stop * 0.8), stop)
    const int cut = (int)((double)(nw + 1) * 0.8);
    if ((p.mode == CN_GSTD_TRAIN && i >= cut) || (p.mode == CN_GSTD_VAL && i < cut)) return false;
    bool ok = true;
    double prev = 0.0;
    for (int k = 0; k < p.T; ++k) {
        const int f = p.frame_list[(size_t)e * p.F + i + k];
        if (f < 0 || f >= p.F) return false;
        const double id = (double)p.frame_id[(size_t)f * p.E + e];
        if (k == 0) fid0 = (float)id;
        else ok = ok && (id - prev == 1.0);   // the window's frames are spaced by frame_diff
        prev = id;
        if (threadIdx.x == 0) w.frames[k] = f;
    }
    return ok;
}

// Ranks the window's ids; -> number of distinct ids; survive = some id has a row in all T frames.  All 64 lanes take part.
__device__ __forceinline__ int gd_rank(const GdArgs &p, int e, GdWindow &w, bool &survive)
{
    const int lane = threadIdx.x, H = p.H, n = p.T * H;
    __syncthreads();
    for (int j = lane; j < n; j += 64) {
        const int k = j / H, h = j - k * H;
        const float4 row = reinterpret_cast<const float4 *>(p.log)[((size_t)w.frames[k] * p.E + e) * H + h];
        w.sid[j] = gd_visible(row.w) ? row.y : __builtin_nanf("");
    }
    __syncthreads();
    int nped = 0;
    bool full = false;
    for (int base = 0; base < n; base += 64) {
        const int j = base + lane;
        const float id = j < n ? w.sid[j] : __builtin_nanf("");
        int same = 0;
        bool first = id == id;
        for (int m = 0; m < n; ++m) {
            const bool eq = w.sid[m] == id;
            same += eq ? 1 : 0;
            first = first && !(eq && m < j);
        }
        if (j < n) w.sfirst[j] = first ? 1 : 0;
        nped += __popcll(__ballot(first));
        full = full || same == p.T;
    }
    survive = __ballot(full) != 0;
    __syncthreads();
    for (int j = lane; j < n; j += 64) {
        const float id = w.sid[j];
        int r = 0;
        for (int m = 0; m < n; ++m) r += (w.sfirst[m] && w.sid[m] < id) ? 1 : 0;
        w.srank[j] = (int16_t)r;
    }
    __syncthreads();
    return nped;
}

// ---- pass 1c: one wavefront per candidate: pedestrians of the sequence it becomes (0 = none), its first frame id ----
__global__ __launch_bounds__(64) void gd_count_kernel(GdArgs p, int32_t *__restrict__ ped_count, float *__restrict__ first_frame,
                                                      int32_t *__restrict__ status)
{
    __shared__ GdWindow w;
    const int cand = blockIdx.x;
    int e, count = 0;
    float fid0 = 0.0f;
    if (gd_candidate(p, cand, w, e, fid0)) {
        bool survive;
        const int nped = gd_rank(p, e, w, survive);
        if (survive) {
            if (nped > CN_MAX_HUMANS) { if (threadIdx.x == 0) atomicOr(status, (int)CN_GSTD_TOO_MANY_PEDS); }
            else count = nped;
        }
    }
    if (threadIdx.x == 0) { ped_count[cand] = count; first_frame[cand] = fid0; }
}

struct GdOut {
    const int32_t *ped_count, *ped_offset;
    int64_t total_peds;
    float *obs_traj, *pred_traj, *obs_traj_rel, *pred_traj_rel, *loss_mask, *loss_mask_rel;
};

// ---- pass 2: one wavefront per candidate that became a sequence: its rows of the six arrays ----
__global__ __launch_bounds__(64) void gd_fill_kernel(GdArgs p, GdOut o)
{
    __shared__ GdWindow w;
    __shared__ float spos[CN_MAX_HUMANS * GD_TMAX * 2];
    __shared__ uint8_t spres[CN_MAX_HUMANS * GD_TMAX];
    const int cand = blockIdx.x, lane = threadIdx.x;
    const int count = o.ped_count[cand];
    if (count <= 0 || count > CN_MAX_HUMANS) return;
    const int64_t p0 = o.ped_offset[cand];
    if (p0 < 0 || p0 + count > o.total_peds) return;
    int e;
    float fid0;
    if (!gd_candidate(p, cand, w, e, fid0)) return;
    bool survive;
    const int nped = gd_rank(p, e, w, survive);
    if (!survive || nped != count) return;      // cannot happen: the count pass ran the same code on the same log
    const int T = p.T;
    for (int q = lane; q < count * T; q += 64) { spos[2 * q] = GD_INVALID; spos[2 * q + 1] = GD_INVALID; spres[q] = 0; }
    __syncthreads();
    const int H = p.H, n = T * H, GP = T - GD_OBS;
    for (int j = lane; j < n; j += 64) {
        if (!(w.sid[j] == w.sid[j])) continue;
        const int k = j / H, h = j - k * H, col = w.srank[j];
        const float4 row = reinterpret_cast<const float4 *>(p.log)[((size_t)w.frames[k] * p.E + e) * H + h];
        if (col < count) { spos[(col * T + k) * 2] = row.z; spos[(col * T + k) * 2 + 1] = row.w; spres[col * T + k] = 1; }
    }
    __syncthreads();
    for (int q = lane; q < count * 2 * T; q += 64) {
        const int ped = q / (2 * T), r = q - ped * 2 * T, c = r / T, t = r - c * T;
        const float x = spos[(ped * T + t) * 2 + c];
        const bool here = spres[ped * T + t] != 0;
        const bool before = t > 0 && spres[ped * T + t - 1] != 0;
        const bool has_rel = t == 0 ? here : (here && before);
        float rel = GD_INVALID;
        if (has_rel) rel = t == 0 ? 0.0f : (float)((double)x - (double)spos[(ped * T + t - 1) * 2 + c]);
        const size_t half = (size_t)(p0 + ped) * 2 + c;   // obs arrays [total_peds,2,5], pred arrays [total_peds,2,P]
        if (t < GD_OBS) { o.obs_traj[half * GD_OBS + t] = x; o.obs_traj_rel[half * GD_OBS + t] = rel; }
        else { o.pred_traj[half * GP + t - GD_OBS] = x; o.pred_traj_rel[half * GP + t - GD_OBS] = rel; }
        if (c == 0) {
            o.loss_mask[(size_t)(p0 + ped) * T + t] = here ? 1.0f : 0.0f;
            o.loss_mask_rel[(size_t)(p0 + ped) * T + t] = has_rel ? 1.0f : 0.0f;
        }
    }
}

// ---- minibatch assembly: one workgroup per sequence of the batch ----
struct GbArgs {
    int B, Np, S, P;           // P: predicted steps (v_pred [B,P,Np,2], masks [.,5 + P])
    int64_t total_peds;
    const int32_t *index, *seq_start, *seq_count;
    const float *cos_sin, *obs_traj_rel, *pred_traj_rel, *loss_mask_rel;
    float *v_obs, *v_pred, *mask_out;
};

__global__ __launch_bounds__(256) void gd_gather_kernel(GbArgs p)
{
    const int b = blockIdx.x, Np = p.Np;
    const int s = p.index[b];
    int count = 0;
    int64_t p0 = 0;
    if (s >= 0 && s < p.S) {
        count = p.seq_count[s]; p0 = p.seq_start[s];
        count = count < 0 ? 0 : (count > Np ? Np : count);
        if (p0 < 0 || p0 + count > p.total_peds) count = 0;
    }
    const bool rot = p.cos_sin != nullptr;
    const float cs = rot ? p.cos_sin[2 * b] : 1.0f, sn = rot ? p.cos_sin[2 * b + 1] : 0.0f;
    const int nv = GD_OBS * Np * 2, nvp = p.P * Np * 2, T = GD_OBS + p.P;
    // v[b, t, n, c] = rel[p0 + n, c, t] (seq_to_graph), rotated (rotate_graph) or copied; zeros at and beyond the sequence's crowd
    for (int q = threadIdx.x; q < nv + nvp; q += blockDim.x) {
        const bool pred = q >= nv;
        const int r = pred ? q - nv : q, steps = pred ? p.P : GD_OBS;
        const int t = r / (2 * Np), n = (r >> 1) % Np, c = r & 1;
        float v = 0.0f;
        if (n < count) {
            const float *src = (pred ? p.pred_traj_rel : p.obs_traj_rel) + (size_t)(p0 + n) * 2 * steps;
            const float x = src[t], y = src[steps + t];
            if (!rot) v = c == 0 ? x : y;
            else v = c == 0 ? x * cs - y * sn : x * sn + y * cs;
        }
        (pred ? p.v_pred + (size_t)b * nvp : p.v_obs + (size_t)b * nv)[r] = v;
    }
    for (int q = threadIdx.x; q < Np * T; q += blockDim.x) {
        const int n = q / T;
        p.mask_out[(size_t)b * Np * T + q] = n < count ? p.loss_mask_rel[(size_t)p0 * T + q] : 0.0f;
    }
}

bool gd_shape_ok(int F, int E, int H, int P)
{
    return P >= 1 && P <= CN_MAX_PRED && F >= GD_OBS + P && E >= 1 && H >= 1 && H <= CN_MAX_HUMANS && (long long)F * E < (1LL << 24);
}
#define GD_REQUIRE_SHAPE(who) \
    CN_REQUIRE(gd_shape_ok(F, E, H, P), who ": F=%d samples (at least 5 + P = %d), E=%d envs, H=%d rows (1..%d), F*E < 2^24, P=%d predicted steps (1..%d)", \
               F, GD_OBS + P, E, H, CN_MAX_HUMANS, P, CN_MAX_PRED)

} // namespace

extern "C" int cn_gst_data_frames_horizon(int F, int E, int H, int P, const float *log, int32_t *visible, float *frame_id, int32_t *status, void *stream)
{
    GD_REQUIRE_SHAPE("cn_gst_data_frames");
    CN_REQUIRE(log && visible && frame_id && status, "cn_gst_data_frames: log, visible, frame_id and status are required");
    CN_REQUIRE(((uintptr_t)log & 15u) == 0, "cn_gst_data_frames: log must be 16-byte aligned");
    hipLaunchKernelGGL(gd_frames_kernel, dim3((unsigned)(F * E)), dim3(64), 0, (hipStream_t)stream, F * E, H, reinterpret_cast<const float4 *>(log), visible,
                       frame_id, status);
    CN_CHECK_LAUNCH();
    return CN_OK;
}

extern "C" int cn_gst_data_count_horizon(int F, int E, int H, int mode, int P, const float *log, const int32_t *visible, const int32_t *listed_before,
                                         const float *frame_id, int32_t *frame_list, int32_t *ped_count, float *first_frame, int32_t *status, void *stream)
{
    GD_REQUIRE_SHAPE("cn_gst_data_count");
    CN_REQUIRE(mode >= CN_GSTD_ALL && mode <= CN_GSTD_VAL, "cn_gst_data_count: mode %d", mode);
    CN_REQUIRE(log && visible && listed_before && frame_id && frame_list && ped_count && first_frame && status, "cn_gst_data_count: every buffer is required");
    CN_REQUIRE(((uintptr_t)log & 15u) == 0, "cn_gst_data_count: log must be 16-byte aligned");
    const hipStream_t st = (hipStream_t)stream;
    const int FE = F * E;
    CN_HIP(hipMemsetAsync(frame_list, 0xff, sizeof(int32_t) * (size_t)FE, st));       // -1: no such listed frame
    hipLaunchKernelGGL(gd_compact_kernel, dim3((unsigned)((FE + 255) / 256)), dim3(256), 0, st, F, E, visible, listed_before, frame_list);
    CN_CHECK_LAUNCH();
    hipLaunchKernelGGL(gd_order_kernel, dim3((unsigned)((FE + 255) / 256)), dim3(256), 0, st, F, E, visible, listed_before, frame_list, frame_id, status);
    CN_CHECK_LAUNCH();
    GdArgs p;
    p.F = F; p.E = E; p.H = H; p.T = GD_OBS + P; p.W = F - (p.T - 1); p.mode = mode;
    p.log = log; p.visible = visible; p.listed_before = listed_before; p.frame_list = frame_list; p.frame_id = frame_id;
    hipLaunchKernelGGL(gd_count_kernel, dim3((unsigned)(E * p.W)), dim3(64), 0, st, p, ped_count, first_frame, status);
    CN_CHECK_LAUNCH();
    return CN_OK;
}

extern "C" int cn_gst_data_fill_horizon(int F, int E, int H, int mode, int P, const float *log, const int32_t *visible, const int32_t *listed_before,
                                        const float *frame_id, const int32_t *frame_list, const int32_t *ped_count, const int32_t *ped_offset,
                                        int64_t total_peds, float *obs_traj, float *pred_traj, float *obs_traj_rel, float *pred_traj_rel, float *loss_mask,
                                        float *loss_mask_rel, void *stream)
{
    GD_REQUIRE_SHAPE("cn_gst_data_fill");
    CN_REQUIRE(mode >= CN_GSTD_ALL && mode <= CN_GSTD_VAL, "cn_gst_data_fill: mode %d", mode);
    CN_REQUIRE(total_peds >= 1 && total_peds < (1LL << 31), "cn_gst_data_fill: total_peds=%lld outside [1, 2^31)", (long long)total_peds);
    CN_REQUIRE(log && visible && listed_before && frame_id && frame_list && ped_count && ped_offset && obs_traj && pred_traj && obs_traj_rel &&
                   pred_traj_rel && loss_mask && loss_mask_rel, "cn_gst_data_fill: every buffer is required");
    CN_REQUIRE(((uintptr_t)log & 15u) == 0, "cn_gst_data_fill: log must be 16-byte aligned");
    GdArgs p;
    p.F = F; p.E = E; p.H = H; p.T = GD_OBS + P; p.W = F - (p.T - 1); p.mode = mode;
    p.log = log; p.visible = visible; p.listed_before = listed_before; p.frame_list = frame_list; p.frame_id = frame_id;
    GdOut o;
    o.ped_count = ped_count; o.ped_offset = ped_offset; o.total_peds = total_peds;
    o.obs_traj = obs_traj; o.pred_traj = pred_traj; o.obs_traj_rel = obs_traj_rel; o.pred_traj_rel = pred_traj_rel;
    o.loss_mask = loss_mask; o.loss_mask_rel = loss_mask_rel;
    hipLaunchKernelGGL(gd_fill_kernel, dim3((unsigned)(E * p.W)), dim3(64), 0, (hipStream_t)stream, p, o);
    CN_CHECK_LAUNCH();
    return CN_OK;
}

extern "C" int cn_gst_gather_batch_horizon(int B, int Np, int P, int num_seq, int64_t total_peds, const int32_t *index, const float *cos_sin,
                                           const int32_t *seq_start, const int32_t *seq_count, const float *obs_traj_rel, const float *pred_traj_rel,
                                           const float *loss_mask_rel, float *v_obs, float *v_pred, float *loss_mask_rel_out, void *stream)
{
    CN_REQUIRE(B >= 1 && B < (1 << 24), "cn_gst_gather_batch: B=%d sequences", B);
    CN_REQUIRE(Np >= 4 && Np <= CN_MAX_HUMANS, "cn_gst_gather_batch: Np=%d outside [4,%d]", Np, CN_MAX_HUMANS);
    CN_REQUIRE(P >= 1 && P <= CN_MAX_PRED, "cn_gst_gather_batch: P=%d predicted steps outside [1,%d]", P, CN_MAX_PRED);
    CN_REQUIRE(num_seq >= 1 && total_peds >= 1 && total_peds < (1LL << 31), "cn_gst_gather_batch: a dataset of %d sequences / %lld pedestrians", num_seq, (long long)total_peds);
    CN_REQUIRE(index && seq_start && seq_count && obs_traj_rel && pred_traj_rel && loss_mask_rel && v_obs && v_pred && loss_mask_rel_out,
               "cn_gst_gather_batch: every buffer but cos_sin is required");
    GbArgs p;
    p.B = B; p.Np = Np; p.S = num_seq; p.P = P; p.total_peds = total_peds;
    p.index = index; p.seq_start = seq_start; p.seq_count = seq_count; p.cos_sin = cos_sin;
    p.obs_traj_rel = obs_traj_rel; p.pred_traj_rel = pred_traj_rel; p.loss_mask_rel = loss_mask_rel;
    p.v_obs = v_obs; p.v_pred = v_pred; p.mask_out = loss_mask_rel_out;
    hipLaunchKernelGGL(gd_gather_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, p);
    CN_CHECK_LAUNCH();
    return CN_OK;
}

// the entry points without a horizon: P = 5, the same launches
extern "C" int cn_gst_data_frames(int F, int E, int H, const float *log, int32_t *visible, float *frame_id, int32_t *status, void *stream)
{
    return cn_gst_data_frames_horizon(F, E, H, 5, log, visible, frame_id, status, stream);
}
extern "C" int cn_gst_data_count(int F, int E, int H, int mode, const float *log, const int32_t *visible, const int32_t *listed_before,
                                 const float *frame_id, int32_t *frame_list, int32_t *ped_count, float *first_frame, int32_t *status, void *stream)
{
    return cn_gst_data_count_horizon(F, E, H, mode, 5, log, visible, listed_before, frame_id, frame_list, ped_count, first_frame, status, stream);
}
extern "C" int cn_gst_data_fill(int F, int E, int H, int mode, const float *log, const int32_t *visible, const int32_t *listed_before,
                                const float *frame_id, const int32_t *frame_list, const int32_t *ped_count, const int32_t *ped_offset,
                                int64_t total_peds, float *obs_traj, float *pred_traj, float *obs_traj_rel, float *pred_traj_rel, float *loss_mask,
                                float *loss_mask_rel, void *stream)
{
    return cn_gst_data_fill_horizon(F, E, H, mode, 5, log, visible, listed_before, frame_id, frame_list, ped_count, ped_offset, total_peds, obs_traj, pred_traj,
                                    obs_traj_rel, pred_traj_rel, loss_mask, loss_mask_rel, stream);
}
extern "C" int cn_gst_gather_batch(int B, int Np, int num_seq, int64_t total_peds, const int32_t *index, const float *cos_sin, const int32_t *seq_start,
                                   const int32_t *seq_count, const float *obs_traj_rel, const float *pred_traj_rel, const float *loss_mask_rel,
                                   float *v_obs, float *v_pred, float *loss_mask_rel_out, void *stream)
{
    return cn_gst_gather_batch_horizon(B, Np, 5, num_seq, total_peds, index, cos_sin, seq_start, seq_count, obs_traj_rel, pred_traj_rel, loss_mask_rel, v_obs,
                                       v_pred, loss_mask_rel_out, stream);
}
