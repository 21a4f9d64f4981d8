// cvr_svdsmall.cpp -- the small dense singular value decomposition behind cvr_svd_host (include/cvr_amd.h): the one-sided cyclic Jacobi method of
// Hestenes (J. SIAM 6, 1958) by rows, plain C++ on the host, for the projected matrix of cvr_svds_device (p <= q <= CVR_SVD_MAX_NCV + 1).
// Every operation is in fp64 in a fixed order: the same input gives the same bits every time.  The wrapper that checks the arguments and sets
// cvr_last_error is in cvr_svds.hip; this file stands alone, like its sibling cvr_symeig.cpp.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <numeric>

#include "../../include/cvr_amd.h"

namespace cvrh {

// B (p x q, p <= q, element (i, j) at b[i + j * ldb], every element finite) = Q diag(s) P^T: s descending, Q (p x p) at uq, P (q x p) at vp (either
// may be null).  The rows of B are the columns g_i of G = B^T; plane rotations from the right make them orthogonal, G J = W: then s_i = ||w_i||,
// P = W diag(1 / s) and Q = J.  0: done; 1: the sweeps ran out.
int svd_small(int p, int q, const double *b, int ldb, double *s, double *uq, int lduq, double *vp, int ldvp)
{
    constexpr int    M = CVR_SVD_MAX_NCV + 1, kSweeps = 60;
    constexpr double kEps = 2.220446049250313e-16;
    static thread_local double g[M][M], jm[M][M];          // g[i]: row i of B (q values); jm[i]: column i of J (p values)
    double                     nrm[M];
    // a power of two takes the largest magnitude into [0.5, 1): exact, and the squares below neither overflow nor vanish
    double big = 0;
    for (int j = 0; j < q; j++)
        for (int i = 0; i < p; i++) big = std::max(big, std::fabs(b[(size_t)j * ldb + i]));
    int ex = 0;
    if (big > 0) (void)std::frexp(big, &ex);
    for (int i = 0; i < p; i++) {
        for (int j = 0; j < q; j++) g[i][j] = std::ldexp(b[(size_t)j * ldb + i], -ex);
        for (int j = 0; j < p; j++) jm[i][j] = i == j ? 1.0 : 0.0;
    }
    auto dot = [&](const double *x, const double *y, int n) {
        double a = 0;
        for (int l = 0; l < n; l++) a += x[l] * y[l];
        return a;
    };
    // a row whose norm is below 2^-52 of the matrix's Frobenius norm (which the rotations keep) is a zero singular value to working precision: it is
    // left alone, or rounding noise would be rotated against rounding noise sweep after sweep (equal rows leave such a row behind)
    double fro2 = 0;
    for (int i = 0; i < p; i++) fro2 += dot(g[i], g[i], q);
    const double floor2 = kEps * kEps * fro2;
    bool done = p <= 1 || big == 0;
    for (int sweep = 1; sweep <= kSweeps && !done; sweep++) {
        int rotated = 0;
        for (int i = 0; i + 1 < p; i++)
            for (int j = i + 1; j < p; j++) {
                const double a = dot(g[i], g[i], q), c = dot(g[j], g[j], q), d = dot(g[i], g[j], q);
                if (!(a > floor2 && c > floor2) || !(std::fabs(d) > kEps * std::sqrt(a * c))) continue;          // a negligible row, or orthogonal to working precision
                rotated++;
                const double zeta = (c - a) / (2.0 * d);
                double       t = 1.0 / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
                if (zeta < 0) t = -t;
                // (x, y) -> (cs x - sn y, sn x + cs y) in Rutishauser's form, as in cvr_symeig.cpp: cs = 1 - sn * tau is never rounded on its own
                const double cs = 1.0 / std::sqrt(1.0 + t * t), sn = cs * t, tau = sn / (1.0 + cs);
                auto         rot = [&](double &x, double &y) {
                    const double gx = x, hy = y;
                    x = gx - sn * (hy + gx * tau);
                    y = hy + sn * (gx - hy * tau);
                };
                for (int l = 0; l < q; l++) rot(g[i][l], g[j][l]);
                for (int l = 0; l < p; l++) rot(jm[i][l], jm[j][l]);
            }
        done = rotated == 0;
    }
    for (int i = 0; i < p; i++) nrm[i] = std::sqrt(dot(g[i], g[i], q));
    // descending; equal values in the order of the rows they ended at
    int order[M];
    std::iota(order, order + p, 0);
    std::stable_sort(order, order + p, [&](int x, int y) { return nrm[x] > nrm[y]; });
    // the right vectors: w_i / s_i; where s_i is zero to working precision the direction of w_i is noise, and the column is completed instead (below)
    const double tiny = (double)q * kEps * (p ? nrm[order[0]] : 0.0);
    static thread_local double pv[M][M];          // pv[c]: column c of P (q values)
    bool                       have[M];
    for (int c = 0; c < p; c++) {
        const int src = order[c];
        have[c] = nrm[src] > tiny;
        if (have[c])
            for (int l = 0; l < q; l++) pv[c][l] = g[src][l] / nrm[src];
    }
    for (int c = 0; c < p; c++) {
        if (have[c]) continue;
        // the unit vector that the columns so far leave most of (the first of them), orthogonalised against them twice
        int    best = 0;
        double left = -1;
        for (int l = 0; l < q; l++) {
            double r = 1.0;
            for (int k = 0; k < p; k++)
                if (have[k]) r -= pv[k][l] * pv[k][l];
            if (r > left) { left = r; best = l; }
        }
        for (int l = 0; l < q; l++) pv[c][l] = l == best ? 1.0 : 0.0;
        for (int pass = 0; pass < 2; pass++)
            for (int k = 0; k < p; k++) {
                if (!have[k]) continue;
                const double h = dot(pv[k], pv[c], q);
                for (int l = 0; l < q; l++) pv[c][l] -= h * pv[k][l];
            }
        const double n2 = std::sqrt(dot(pv[c], pv[c], q));
        for (int l = 0; l < q; l++) pv[c][l] /= n2;
        have[c] = true;
    }
    for (int c = 0; c < p; c++) {
        const int src = order[c];
        s[c] = std::ldexp(nrm[src], ex);
        // the sign: the component of largest magnitude of the left vector (the first of them) is positive
        int top = 0;
        for (int i = 1; i < p; i++)
            if (std::fabs(jm[src][i]) > std::fabs(jm[src][top])) top = i;
        const bool flip = jm[src][top] < 0;
        if (uq)
            for (int i = 0; i < p; i++) uq[(size_t)c * lduq + i] = flip ? -jm[src][i] : jm[src][i];
        if (vp)
            for (int l = 0; l < q; l++) vp[(size_t)c * ldvp + l] = flip ? -pv[c][l] : pv[c][l];
    }
    return done ? 0 : 1;
}

}  // namespace cvrh
