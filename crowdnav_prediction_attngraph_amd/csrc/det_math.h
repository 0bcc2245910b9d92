// det_math.h -- deterministic fp64 sin/cos, exp and log from +,-,*,/ only (bit-reproducible against the oracle's twins), and the
// field-of-view test of detect_visible.  Part of env_sim.hip's translation unit (compiled with -ffp-contract=off).
#pragma once
#include "common.h"

#include <cmath>

namespace {

// ------------------------------------------------------------------------------------------------------------------
// deterministic sin/cos on [0, 2*pi]: Cody-Waite reduction by pi/2 + minimax kernels, +,-,* only.  Stands in for
// np.cos/np.sin (crowd_sim_var_num.py:127-128); documented in DESIGN.md (<= 1 ulp from libm).
// ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double poly_sin(double x)
{
    const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
                 S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    const double z = x * x, w = z * z;
    const double r = S2 + z * (S3 + z * S4) + z * w * (S5 + z * S6);
    const double v = z * x;
    return x + v * (S1 + z * r);
}
__device__ __forceinline__ double poly_cos(double x)
{
    const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05,
                 C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    const double z = x * x;
    double w = z * z;
    const double r = z * (C1 + z * (C2 + z * C3)) + (w * w) * (C4 + z * (C5 + z * C6));
    const double hz = 0.5 * z;
    w = 1.0 - hz;
    return w + (((1.0 - w) - hz) + z * r);
}
__device__ __forceinline__ void det_sincos(double x, double &s, double &c)
{
    const double INV_PIO2 = 6.36619772367581382433e-01, PIO2_1 = 1.57079632673412561417e+00,
                 PIO2_1T = 6.07710050650619224932e-11;
    const int k = (int)(x * INV_PIO2 + 0.5);
    const double fk = (double)k;
    const double r = (x - fk * PIO2_1) - fk * PIO2_1T;
    const double sr = poly_sin(r), cr = poly_cos(r);
    switch (k & 3) {
    case 0: s = sr; c = cr; break;
    case 1: s = cr; c = -sr; break;
    case 2: s = -sr; c = -cr; break;
    default: s = -cr; c = sr; break;
    }
}

// deterministic exp: Cody-Waite reduction by ln 2 + degree-5 minimax kernel, +,-,*,/ only; the twin of the oracle's orc_exp.
// Stands in for np.exp in the social-force policy (crowd_nav/policy/social_force.py:37).
__device__ __forceinline__ double det_exp(double x)
{
    const double LN2_HI = 6.93147180369123816490e-01, LN2_LO = 1.90821492927058770002e-10, INV_LN2 = 1.44269504088896338700e+00;
    const double P1 = 1.66666666666666019037e-01, P2 = -2.77777777770155933842e-03, P3 = 6.61375632143793436117e-05,
                 P4 = -1.65339022054652515390e-06, P5 = 4.13813679705723846039e-08;
    if (x > 700.0) x = 700.0;
    if (x < -700.0) return 0.0;
    const int k = (int)(INV_LN2 * x + (x < 0.0 ? -0.5 : 0.5));
    const double fk = (double)k;
    const double hi = x - fk * LN2_HI, lo = fk * LN2_LO;
    const double r = hi - lo;
    const double t = r * r;
    const double c = r - t * (P1 + t * (P2 + t * (P3 + t * (P4 + t * P5))));
    const double y = 1.0 - ((lo - (r * c) / (2.0 - c)) - hi);
    return ldexp(y, k);
}

// deterministic natural logarithm for normal positive arguments (classic reduction to sqrt(2)/2 < 1 + f < sqrt(2), degree-14 minimax in
// s = f / (2 + f)); the twin of the oracle's orc_log.  Stands in for log() in RandomState.normal's polar method (arguments in (0, 1)).
__device__ __forceinline__ double det_log(double x)
{
    const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10;
    const double Lg1 = 6.666666666666735130e-01, Lg2 = 3.999999999940941908e-01, Lg3 = 2.857142874366239149e-01, Lg4 = 2.222219843214978396e-01,
                 Lg5 = 1.818357216161805012e-01, Lg6 = 1.531383769920937332e-01, Lg7 = 1.479819860511658591e-01;
    unsigned long long bits = (unsigned long long)__double_as_longlong(x);
    int hx = (int)(bits >> 32);
    int k = (hx >> 20) - 1023;
    hx &= 0x000fffff;
    const int i0 = (hx + 0x95f64) & 0x100000;
    bits = ((unsigned long long)(unsigned)(hx | (i0 ^ 0x3ff00000)) << 32) | (bits & 0xffffffffull);
    x = __longlong_as_double((long long)bits);
    k += i0 >> 20;
    const double f = x - 1.0;
    const double dk = (double)k;
    if ((0x000fffff & (2 + hx)) < 3) {
        if (f == 0.0) return k == 0 ? 0.0 : dk * ln2_hi + dk * ln2_lo;
        const double R0 = f * f * (0.5 - 0.33333333333333333 * f);
        return k == 0 ? f - R0 : dk * ln2_hi - ((R0 - dk * ln2_lo) - f);
    }
    const double s = f / (2.0 + f);
    const double z = s * s;
    const double w = z * z;
    const double t1 = w * (Lg2 + w * (Lg4 + w * Lg6));
    const double t2 = z * (Lg1 + w * (Lg3 + w * (Lg5 + w * Lg7)));
    const double R = t2 + t1;
    const int i = (hx - 0x6147a) | (0x6b851 - hx);
    if (i > 0) {
        const double hfsq = 0.5 * f * f;
        return k == 0 ? f - (hfsq - s * (hfsq + R)) : dk * ln2_hi - ((hfsq - (s * (hfsq + R) + dk * ln2_lo)) - f);
    }
    return k == 0 ? f - s * (f - R) : dk * ln2_hi - ((s * (f - R) - dk * ln2_lo) - f);
}

// The field-of-view half of detect_visible (crowd_sim.py:513-537): agent 2 inside agent 1's cone of fov * pi radians around agent 1's
// heading -- the direction of its velocity when the robot is holonomic (at rest: +x, or -x for vx = -0.0, as np.arctan2 has it), its theta
// otherwise.  Decision-equivalent form of arccos(clip(v_fov . v_12)) <= fov / 2 (see the oracle's in_fov for why); coincident agents
// give NaN and are not visible.
template <class C>
__device__ __forceinline__ bool in_fov(const C &c, double fov, double px1, double py1, double vx1, double vy1, double theta1,
                                       double px2, double py2)
{
    double fx, fy;
    if (c.kinematics == CN_KIN_UNICYCLE) det_sincos(theta1, fy, fx);
    else if (vx1 == 0.0 && vy1 == 0.0) { fx = __double_as_longlong(vx1) < 0 ? -1.0 : 1.0; fy = 0.0; }
    else { const double nv = sqrt(vx1 * vx1 + vy1 * vy1); fx = vx1 / nv; fy = vy1 / nv; }
    const double dx = px2 - px1, dy = py2 - py1;
    const double n12 = sqrt(dx * dx + dy * dy);
    double d = fx * (dx / n12) + fy * (dy / n12);
    d = d < -1.0 ? -1.0 : (d > 1.0 ? 1.0 : d); // keeps NaN, like np.clip
    const double half = M_PI * fov / 2.0;
    double thr = -1.0;
    if (half < M_PI) { double sn; det_sincos(half, sn, thr); }
    return d >= thr;
}

} // namespace
