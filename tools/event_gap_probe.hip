// Probe: what does releasing a side stream cost the CALLER's stream?  Two ~20 us kernels back to back on one stream; a second, lowest-priority
// non-blocking stream runs a small kernel that depends on the first one (as the env batch's side stream depends on env_step / orca_lane).
// Every kernel stamps the device clock (s_memrealtime, 10 ns ticks) at entry and exit.  Reported per case, medians over REPS repetitions:
// the gap end of kernel 1 -> start of kernel 2, and how long after kernel 1's end the dependent kernel starts.
//   (a) nothing between the two kernels (and no dependent)
//   (b) hipEventRecord(ev, main) + hipStreamWaitEvent(side, ev) between them
//   (c) kernel 1 launched through hipExtLaunchKernelGGL with ev as its stop event, then hipStreamWaitEvent(side, ev): no record.
//       (the hope: a bound stop event rides on the kernel's own dispatch packet instead of a marker packet behind it)
//   (d) hipStreamWriteValue64(main, word, epoch) between them, hipStreamWaitValue64(side, word, epoch, gte) enqueued after it
//   (e), (f): (c) and (b) with an event created with hipEventDisableTiming | hipEventReleaseToDevice (no system-scope release behind kernel 1)
// hipcc --offload-arch=gfx950 -O2 -o event_gap_probe event_gap_probe.hip
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s -> %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)
constexpr int REPS = 200, WARM = 20, SLOTS = 8;
__global__ void spin(long long ticks, long long *t)
{
    const long long t0 = wall_clock64();
    if (threadIdx.x == 0) t[0] = t0;
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(4);
    if (threadIdx.x == 0) t[1] = wall_clock64();
}
static double median(std::vector<double> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }
static double pct(std::vector<double> v, double p) { std::sort(v.begin(), v.end()); return v[(size_t)(p * (v.size() - 1))]; }
int main()
{
    int least = 0, greatest = 0;
    CK(hipDeviceGetStreamPriorityRange(&least, &greatest));
    hipStream_t mainst, side;
    CK(hipStreamCreateWithFlags(&mainst, hipStreamNonBlocking));
    CK(hipStreamCreateWithPriority(&side, hipStreamNonBlocking, least));
    hipEvent_t ev, ev_back;
    CK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    CK(hipEventCreateWithFlags(&ev_back, hipEventDisableTiming));
    hipEvent_t ev_sys = ev, ev_dev;
    CK(hipEventCreateWithFlags(&ev_dev, hipEventDisableTiming | hipEventReleaseToDevice));
    const size_t words = (size_t)(REPS + WARM) * SLOTS;
    long long *t; CK(hipMalloc(&t, words * 8));
    unsigned long long *gate; CK(hipMalloc(&gate, 256)); CK(hipMemset(gate, 0, 256));
    std::vector<long long> h(words);
    unsigned long long epoch = 0;
    const long long K = 2000; // 20 us
    for (int cc = 0; cc < 6; ++cc) {
        const int c = cc == 4 ? 2 : cc == 5 ? 1 : cc;
        ev = cc >= 4 ? ev_dev : ev_sys;
        CK(hipMemset(t, 0, words * 8));
        CK(hipDeviceSynchronize());
        for (int r = 0; r < REPS + WARM; ++r) {
            long long *tr = t + (size_t)r * SLOTS;
            if (c == 2) hipExtLaunchKernelGGL(spin, dim3(1), dim3(64), 0, mainst, nullptr, ev, 0, K, tr);
            else hipLaunchKernelGGL(spin, dim3(1), dim3(64), 0, mainst, K, tr);
            CK(hipGetLastError());
            if (c == 1) CK(hipEventRecord(ev, mainst));
            if (c == 1 || c == 2) CK(hipStreamWaitEvent(side, ev, 0));
            if (c == 3) {
                ++epoch;
                CK(hipStreamWriteValue64(mainst, gate, epoch, 0));
                CK(hipStreamWaitValue64(side, gate, epoch, hipStreamWaitValueGte, 0xffffffffffffffffull));
            }
            hipLaunchKernelGGL(spin, dim3(1), dim3(64), 0, mainst, K, tr + 2);
            CK(hipGetLastError());
            if (c != 0) {
                // the dependent: short, and the next repetition waits for it as the next sim step waits for the ORCA tail
                hipLaunchKernelGGL(spin, dim3(1), dim3(64), 0, side, 200LL, tr + 4);
                CK(hipGetLastError());
                CK(hipEventRecord(ev_back, side));
                CK(hipStreamWaitEvent(mainst, ev_back, 0));
            }
        }
        CK(hipDeviceSynchronize());
        CK(hipMemcpy(h.data(), t, words * 8, hipMemcpyDeviceToHost));
        std::vector<double> gap, dep, k1;
        for (int r = WARM; r < REPS + WARM; ++r) {
            const long long *tr = h.data() + (size_t)r * SLOTS;
            gap.push_back((tr[2] - tr[1]) * 0.01);
            k1.push_back((tr[1] - tr[0]) * 0.01);
            if (c != 0) dep.push_back((tr[4] - tr[1]) * 0.01);
        }
        static const char *names[6] = {"(a) nothing between", "(b) event record + wait", "(c) stop event on kernel 1 + wait", "(d) write-value + wait-value",
                                       "(e) as (c), device-scope event", "(f) as (b), device-scope event"};
        printf("%-36s gap k1 end -> k2 start: median %6.2f us (p10 %6.2f, p90 %6.2f)   k1 %5.2f us", names[cc], median(gap), pct(gap, 0.1), pct(gap, 0.9), median(k1));
        if (c != 0) printf("   dependent starts %6.2f us after k1's end (p10 %6.2f, p90 %6.2f)", median(dep), pct(dep, 0.1), pct(dep, 0.9));
        printf("\n");
        fflush(stdout);
    }
    return 0;
}
