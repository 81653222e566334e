// ls_band_map.h -- where the channel band of a footprint starts, by guess and verify (k_project's band_from_ranges, ls_project.hip).
//
// The band's first channel is the lower bound L(t) = first position i with chan_tan_up[i] >= t in the ascending table of
// tan(elevation + margin).  Seven to eight rounds of bisection find it, each a dependent LDS read.  Sensors are close to uniform
// in angle, so position is a smooth function of the tangent: per handle the host fits a cubic x(t) ~ position + 1/2 through the
// table (least squares, in double), and the kernel takes trunc(x(t)) - back as its start, CHECKS it against the table (the entry
// below the start must be below t, else it bisects after all) and walks forward.  The check makes the result exact for any table
// and any rounding of x; the fit only decides how long the walk is.  `back` and `walk` are measured, not assumed: the host runs
// the kernel's own float arithmetic (band_guess below, compiled by both sides) over every table value, its neighbours one ulp
// away, the midpoints, both infinities and values beyond both ends.  A handle whose walk would not be shorter than the bisection
// keeps the bisection (walk < 0).
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define LS_BAND_HD __host__ __device__ __forceinline__
#else
#define LS_BAND_HD inline
#endif

namespace ls {

struct BandMap {
    float a[4];      // x(t) = ((a3 t + a2) t + a1) t + a0, three fused multiply-adds
    float t0, t1;    // t is clamped to the finite range of the table first (-inf, +inf and NaN queries land on t0 / t1 / t0)
    int32_t back;    // start = trunc(x) - back is at or below L(t) for every probed t
    int32_t walk;    // ... and at most this many positions below it; < 0: no map, the kernel bisects
};

// the start position, 0 .. V: the same operation sequence on the device and on the host
LS_BAND_HD uint32_t band_guess(const BandMap &bm, uint32_t V, float t)
{
    const float tc = fminf(fmaxf(t, bm.t0), bm.t1);
    const float x = fmaf(fmaf(fmaf(bm.a[3], tc, bm.a[2]), tc, bm.a[1]), tc, bm.a[0]);   // |x| < 2^24 on [t0, t1] (band_map_fit)
    const int32_t g = (int32_t)x - bm.back;
    return g < 0 ? 0u : ((uint32_t)g > V ? V : (uint32_t)g);
}

// ---- host side: the fit and its judgement ----

inline uint32_t band_lower_bound(const float *up, uint32_t V, float t)
{
    uint32_t lo = 0, hi = V;
    while (lo < hi) { const uint32_t m = (lo + hi) >> 1; if (up[m] < t) lo = m + 1; else hi = m; }
    return lo;
}

// rounds of the bisection over V entries (V + 1 possible answers)
inline int32_t band_bisection_rounds(uint32_t V)
{
    int32_t r = 0;
    for (uint32_t n = V; n; n >>= 1) ++r;
    return r;
}

// the values the fit is judged on: every table entry, one ulp either side, the midpoints, the infinities, beyond both ends
inline std::vector<float> band_map_probes(const float *up, uint32_t V)
{
    std::vector<float> p = {-INFINITY, INFINITY, 0.0f};
    for (uint32_t i = 0; i < V; ++i) {
        p.push_back(up[i]);
        p.push_back(std::nextafter(up[i], -INFINITY));
        p.push_back(std::nextafter(up[i], INFINITY));
        if (i + 1 < V && std::isfinite(up[i]) && std::isfinite(up[i + 1])) p.push_back((float)(0.5 * ((double)up[i] + (double)up[i + 1])));
    }
    if (V && std::isfinite(up[0])) { p.push_back(up[0] - 1.0f); p.push_back(up[0] * 2.0f - 1.0f); p.push_back(-3.0e38f); }
    if (V && std::isfinite(up[V - 1])) { p.push_back(up[V - 1] + 1.0f); p.push_back(up[V - 1] * 2.0f + 1.0f); p.push_back(3.0e38f); }
    return p;
}

// least-squares polynomial (degree <= 3, lower when the table has too few distinct finite values) of position + 1/2 over the
// finite table entries, then back / walk from the probes.  walk < 0 when there is nothing to fit or the walk would not beat
// the bisection: 1 round trip for the check and the first entry + `walk` for the steps against band_bisection_rounds(V).
inline BandMap band_map_fit(const float *up, uint32_t V)
{
    BandMap bm = {{0.0f, 0.0f, 0.0f, 0.0f}, 0.0f, 0.0f, 0, -1};
    std::vector<double> ts, is;
    for (uint32_t i = 0; i < V; ++i)
        if (std::isfinite(up[i])) { ts.push_back(up[i]); is.push_back((double)i + 0.5); }
    if (ts.size() < 2) return bm;
    uint32_t distinct = 1;
    for (size_t k = 1; k < ts.size(); ++k) distinct += ts[k] != ts[k - 1];
    if (distinct < 2) return bm;
    const int deg = (int)std::min<uint32_t>(3u, distinct - 1u), n = deg + 1;
    // normal equations in s = (t - mid) / half, |s| <= 1
    const double mid = 0.5 * (ts.front() + ts.back()), half = 0.5 * (ts.back() - ts.front());
    double A[4][5] = {};
    for (size_t k = 0; k < ts.size(); ++k) {
        const double s = (ts[k] - mid) / half;
        double pw[7] = {1.0, s, s * s, s * s * s, s * s * s * s, s * s * s * s * s, s * s * s * s * s * s};
        for (int r = 0; r < n; ++r) {
            for (int c = 0; c < n; ++c) A[r][c] += pw[r + c];
            A[r][n] += pw[r] * is[k];
        }
    }
    for (int c = 0; c < n; ++c) {   // Gauss-Jordan with partial pivoting
        int piv = c;
        for (int r = c + 1; r < n; ++r) if (std::fabs(A[r][c]) > std::fabs(A[piv][c])) piv = r;
        if (!(std::fabs(A[piv][c]) > 1e-12)) return bm;
        for (int k = 0; k <= n; ++k) std::swap(A[c][k], A[piv][k]);
        for (int r = 0; r < n; ++r) {
            if (r == c) continue;
            const double f = A[r][c] / A[c][c];
            for (int k = c; k <= n; ++k) A[r][k] -= f * A[c][k];
        }
    }
    double cs[4] = {0.0, 0.0, 0.0, 0.0};
    for (int r = 0; r < n; ++r) cs[r] = A[r][n] / A[r][r];
    // x(s(t)) as a polynomial in t: s = u t + w
    const double u = 1.0 / half, w = -mid / half;
    const double at[4] = {cs[0] + cs[1] * w + cs[2] * w * w + cs[3] * w * w * w, cs[1] * u + 2.0 * cs[2] * u * w + 3.0 * cs[3] * u * w * w,
                          cs[2] * u * u + 3.0 * cs[3] * u * u * w, cs[3] * u * u * u};
    const double tmax = std::max(std::fabs(ts.front()), std::fabs(ts.back()));
    double bound = 0.0, pw = 1.0;
    for (int k = 0; k < 4; ++k) { bound += std::fabs(at[k]) * pw; pw *= tmax; }
    if (!(bound < 16777216.0)) return bm;   // (int32_t)x is then defined, and exact
    for (int k = 0; k < 4; ++k) bm.a[k] = (float)at[k];
    bm.t0 = (float)ts.front();
    bm.t1 = (float)ts.back();
    const std::vector<float> probes = band_map_probes(up, V);
    // (more than one pass only where the guess ran into its clamp at V)
    int64_t over = 0;
    for (int pass = 0; pass < 8; ++pass) {
        over = 0;
        for (float t : probes) over = std::max<int64_t>(over, (int64_t)band_guess(bm, V, t) - (int64_t)band_lower_bound(up, V, t));
        if (over <= 0) break;
        bm.back += (int32_t)over;
    }
    if (over > 0) return bm;
    int64_t walk = 0;
    for (float t : probes) walk = std::max<int64_t>(walk, (int64_t)band_lower_bound(up, V, t) - (int64_t)band_guess(bm, V, t));
    bm.walk = 1 + walk < band_bisection_rounds(V) && walk <= 4 ? (int32_t)walk : -1;
    return bm;
}

}  // namespace ls
