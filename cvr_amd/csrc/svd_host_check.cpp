// svd_host_check.cpp -- a stand-alone driver for the small dense SVD (cvr_svdsmall.cpp) under AddressSanitizer and UBSan (make svd-host-asan-check):
// every shape p <= q up to CVR_SVD_MAX_NCV + 1 that the solver can produce, into exactly sized arrays with leading dimensions at their minimum, for
// random, bidiagonal-plus-spike, rank-deficient and zero matrices; null uq / vp; the reconstruction and the orthogonality within a loose bound.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/cvr_amd.h"

namespace cvrh {
int svd_small(int p, int q, const double *b, int ldb, double *s, double *uq, int lduq, double *vp, int ldvp);
}

static uint64_t g_state = 20261021;
static double   rnd()          // in [-1, 1)
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(int64_t)(g_state >> 11) / 4503599627370496.0 - 1.0;
}

static int check(int p, int q, int kind)
{
    std::vector<double> b((size_t)p * q, 0.0), s(p), uq((size_t)p * p), vp((size_t)q * p);
    for (int j = 0; j < q; j++)
        for (int i = 0; i < p; i++) {
            double v = 0;
            if (kind == 0) v = rnd();
            if (kind == 1) v = i == j ? 1.0 + std::fabs(rnd()) : (j == i + 1 || (j == p / 3 && i < p / 3)) ? 0.1 * rnd() : 0.0;
            if (kind == 2) v = (i % 3 == 0 ? 1.0 : 0.0) * (double)((j % 5) + 1);          // rank 1
            b[(size_t)j * p + i] = v;
        }
    if (cvrh::svd_small(p, q, b.data(), p, s.data(), uq.data(), p, vp.data(), q)) return 1;
    std::vector<double> s2(p);
    if (cvrh::svd_small(p, q, b.data(), p, s2.data(), nullptr, 0, nullptr, 0)) return 2;
    double top = s[0] > 0 ? s[0] : 1.0, worst = 0;
    for (int c = 0; c < p; c++) {
        if (s2[c] != s[c] || (c && s[c] > s[c - 1]) || !(s[c] >= 0)) return 3;
        for (int d = 0; d < p; d++) {
            double uu = 0, vv = 0;
            for (int i = 0; i < p; i++) uu += uq[(size_t)c * p + i] * uq[(size_t)d * p + i];
            for (int l = 0; l < q; l++) vv += vp[(size_t)c * q + l] * vp[(size_t)d * q + l];
            worst = std::fmax(worst, std::fmax(std::fabs(uu - (c == d)), std::fabs(vv - (c == d))));
        }
    }
    for (int j = 0; j < q; j++)
        for (int i = 0; i < p; i++) {
            double r = 0;
            for (int c = 0; c < p; c++) r += uq[(size_t)c * p + i] * s[c] * vp[(size_t)c * q + j];
            worst = std::fmax(worst, std::fabs(r - b[(size_t)j * p + i]) / top);
        }
    return worst <= 1e-12 ? 0 : 4;
}

int main()
{
    int bad = 0, runs = 0;
    for (int p = 1; p <= CVR_SVD_MAX_NCV + 1; p += (p < 8 ? 1 : 7))
        for (int q : {p, p + 1, CVR_SVD_MAX_NCV + 1})
            for (int kind = 0; kind < 4; kind++) {
                if (q > CVR_SVD_MAX_NCV + 1) continue;
                const int rc = check(p, q, kind);
                runs++;
                if (rc) {
                    std::printf("svd_small(%d, %d) kind %d: failure %d\n", p, q, kind, rc);
                    bad++;
                }
            }
    std::printf("svd_host_check: %d runs, %d failures\n", runs, bad);
    return bad ? 1 : 0;
}
