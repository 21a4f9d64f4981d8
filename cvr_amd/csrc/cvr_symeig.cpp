// cvr_symeig.cpp -- the small dense symmetric eigensolver behind cvr_sym_eig_host (include/cvr_amd.h): the cyclic Jacobi method by rows in
// Rutishauser's form (Numer. Math. 9, 1966), plain C++ on the host, for the projected matrix of cvr_eigsh_device (m <= CVR_EIG_MAX_NCV).
// Every operation is in fp64 in a fixed order: the same input gives the same bits every time.  The wrapper that checks the arguments and
// sets cvr_last_error is in cvr_lanczos.hip; this file stands alone.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <numeric>

#include "../../include/cvr_amd.h"

namespace cvrh {

// 0: done; 1: the sweeps ran out (an input that is not finite; the caller checks that first)
int sym_eig(int m, const double *a_in, int lda, double *w, double *z, int ldz)
{
    constexpr int M = CVR_EIG_MAX_NCV, kSweeps = 60;
    static thread_local double a[M][M], v[M][M];
    double d[M], b[M], acc[M];
    for (int j = 0; j < m; j++)
        for (int i = j; i < m; i++) a[i][j] = a[j][i] = a_in[(size_t)j * lda + i];          // the lower triangle: (i, j), i >= j, at a[i + j * lda]
    for (int i = 0; i < m; i++) {
        for (int j = 0; j < m; j++) v[i][j] = i == j ? 1.0 : 0.0;
        d[i] = b[i] = a[i][i];
        acc[i] = 0;
    }
    bool done = m <= 1;
    for (int sweep = 1; sweep <= kSweeps && !done; sweep++) {
        double off = 0;
        for (int p = 0; p + 1 < m; p++)
            for (int q = p + 1; q < m; q++) off += std::fabs(a[p][q]);
        if (off == 0) { done = true; break; }
        const double thresh = sweep < 4 ? 0.2 * off / ((double)m * m) : 0.0;
        for (int p = 0; p + 1 < m; p++)
            for (int q = p + 1; q < m; q++) {
                const double apq = a[p][q], g = 100.0 * std::fabs(apq);
                if (sweep > 4 && std::fabs(d[p]) + g == std::fabs(d[p]) && std::fabs(d[q]) + g == std::fabs(d[q])) {
                    a[p][q] = 0;          // too small to move either diagonal entry
                    continue;
                }
                if (!(std::fabs(apq) > thresh)) continue;
                const double diff = d[q] - d[p];
                double       t;
                if (std::fabs(diff) + g == std::fabs(diff)) {
                    t = apq / diff;
                } else {
                    const double theta = 0.5 * diff / apq;
                    t = 1.0 / (std::fabs(theta) + std::sqrt(1.0 + theta * theta));
                    if (theta < 0) t = -t;
                }
                const double c = 1.0 / std::sqrt(1.0 + t * t), s = t * c, tau = s / (1.0 + c), h = t * apq;
                acc[p] -= h; acc[q] += h;
                d[p] -= h; d[q] += h;
                a[p][q] = 0;
                auto rot = [&](double &x, double &y) {
                    const double gx = x, hy = y;
                    x = gx - s * (hy + gx * tau);
                    y = hy + s * (gx - hy * tau);
                };
                for (int j = 0; j < p; j++) rot(a[j][p], a[j][q]);
                for (int j = p + 1; j < q; j++) rot(a[p][j], a[j][q]);
                for (int j = q + 1; j < m; j++) rot(a[p][j], a[q][j]);
                for (int j = 0; j < m; j++) rot(v[j][p], v[j][q]);
            }
        for (int i = 0; i < m; i++) {
            b[i] += acc[i];
            d[i] = b[i];
            acc[i] = 0;
        }
    }
    // ascending; equal values in the order of the diagonal positions they ended at
    int order[M];
    std::iota(order, order + m, 0);
    std::stable_sort(order, order + m, [&](int x, int y) { return d[x] < d[y]; });
    for (int c = 0; c < m; c++) {
        const int src = order[c];
        w[c] = d[src];
        if (!z) continue;
        // the sign: the component of largest magnitude (the first of them) is positive
        int big = 0;
        for (int i = 1; i < m; i++)
            if (std::fabs(v[i][src]) > std::fabs(v[big][src])) big = i;
        const bool flip = v[big][src] < 0;
        for (int i = 0; i < m; i++) z[(size_t)c * ldz + i] = flip ? -v[i][src] : v[i][src];
    }
    return done ? 0 : 1;
}

}  // namespace cvrh
