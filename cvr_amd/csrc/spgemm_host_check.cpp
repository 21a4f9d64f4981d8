// spgemm_host_check.cpp -- a stand-alone driver of the host twin of the sparse matrix-matrix product (cvr_spgemm_host.cpp) for
// `make spgemm-asan-check`: the host code under AddressSanitizer and UBSan on the cases whose index arithmetic differs -- empty matrices (m, k, n or
// nnz 0), empty rows on both sides, duplicates and unsorted rows in A, a cancelling entry, a non-zero first row pointer, fp32 -- in the two-call
// shape with the second call's arrays of exactly nnz entries, and every error return.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cvr_spgemm.h"

// (the library's fail() formats cvr_last_error in cvr_capi.hip, which needs HIP: this one keeps the text for the messages below.  The checks of the
// views are cvr_spgemm_host.cpp's own, check_view: nothing of them is re-implemented here)
namespace cvrh {
static char g_msg[512];
int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_msg, sizeof(g_msg), fmt, ap);
    va_end(ap);
    return code;
}
}  // namespace cvrh

namespace {

struct Csr {
    int64_t              ncols = 0;
    std::vector<int64_t> rp{0};
    std::vector<int32_t> ci;
    std::vector<double>  va;
    explicit Csr(int64_t nc) : ncols(nc) {}
    Csr &row(std::initializer_list<std::pair<int, double>> e)
    {
        for (auto &p : e) {
            ci.push_back(p.first);
            va.push_back(p.second);
        }
        rp.push_back((int64_t)ci.size());
        return *this;
    }
    int64_t nrows() const { return (int64_t)rp.size() - 1; }
};

int failures = 0;

void expect(bool ok, const char *what)
{
    if (!ok) {
        fprintf(stderr, "FAILED: %s (%s)\n", what, cvrh::g_msg);
        failures++;
    }
}

template <typename T>
struct Out {
    int                  rc = 0;
    int64_t              bad = -7;
    std::vector<int64_t> rp;
    std::vector<int32_t> ci;
    std::vector<T>       va;
};

// both calls, the second into arrays of exactly nnz entries; shift: the arrays of A start at row_ptr[0] = shift
template <typename T>
Out<T> run(const Csr &a, const Csr &b, int64_t shift = 0)
{
    std::vector<T>       av(shift, T(9)), bv(b.va.begin(), b.va.end());
    std::vector<int32_t> aci(shift, 0);
    std::vector<int64_t> arp(a.rp);
    for (auto &x : arp) x += shift;
    av.insert(av.end(), a.va.begin(), a.va.end());
    aci.insert(aci.end(), a.ci.begin(), a.ci.end());
    cvr_csr_view va{}, vb{};
    va.nrows = a.nrows();
    va.ncols = a.ncols;
    va.row_ptr = arp.data();
    va.col_idx = aci.data();
    va.vals = av.data();
    vb.nrows = b.nrows();
    vb.ncols = b.ncols;
    vb.row_ptr = b.rp.data();
    vb.col_idx = b.ci.data();
    vb.vals = bv.data();
    va.is_f32 = vb.is_f32 = sizeof(T) == 4;
    Out<T> o;
    o.rp.assign((size_t)a.nrows() + 1, -1);
    o.rc = cvr_spgemm_host(&va, &vb, o.rp.data(), nullptr, nullptr, &o.bad);
    if (o.rc) return o;
    const size_t nnz = (size_t)o.rp.back();
    o.ci.assign(nnz, -1);
    o.va.assign(nnz, T(-1));
    std::vector<int64_t> again(o.rp.size(), -1);
    o.rc = cvr_spgemm_host(&va, &vb, again.data(), nnz ? o.ci.data() : reinterpret_cast<int32_t *>(&o.bad), nnz ? o.va.data() : reinterpret_cast<T *>(&o.bad), &o.bad);
    expect(again == o.rp, "the second call's row_ptr is the first's");
    return o;
}

}  // namespace

int main()
{
    // [1 2; 0 3] * [4 0; 5 6] = [14 12; 15 18], A's first row unsorted
    Csr a(2), b(2);
    a.row({{1, 2.0}, {0, 1.0}}).row({{1, 3.0}});
    b.row({{0, 4.0}}).row({{0, 5.0}, {1, 6.0}});
    auto o = run<double>(a, b);
    expect(o.rc == CVR_OK && o.rp == std::vector<int64_t>({0, 2, 4}) && o.ci == std::vector<int32_t>({0, 1, 0, 1}) && o.va == std::vector<double>({14, 12, 15, 18}), "2 x 2");
    auto f = run<float>(a, b, 5);
    expect(f.rc == CVR_OK && f.va == std::vector<float>({14, 12, 15, 18}), "2 x 2, fp32, row_ptr[0] = 5");
    // duplicates in A and a cancelling entry that stays
    Csr d(2), e(1);
    d.row({{0, 1.0}, {1, -1.0}, {0, 2.0}});
    e.row({{0, 1.0}}).row({{0, 1.0}});
    o = run<double>(d, e);
    expect(o.rc == CVR_OK && o.rp.back() == 1 && o.va[0] == 2.0, "duplicates");
    Csr c1(2);
    c1.row({{0, 1.0}, {1, -1.0}});
    o = run<double>(c1, e);
    expect(o.rc == CVR_OK && o.rp.back() == 1 && o.ci[0] == 0 && o.va[0] == 0.0, "a cancelling entry stays");
    // empty rows on both sides; nnz(A) = 0; nnz(B) = 0; m = 0; k = 0; n = 0
    Csr ea(3), eb(4);
    ea.row({}).row({{1, 1.0}, {2, 1.0}}).row({});
    eb.row({{3, 1.0}}).row({}).row({{0, 2.0}, {3, 1.0}});
    o = run<double>(ea, eb);
    expect(o.rc == CVR_OK && o.rp == std::vector<int64_t>({0, 0, 2, 2}) && o.ci == std::vector<int32_t>({0, 3}), "empty rows");
    Csr za(3), zb(4);
    za.row({}).row({});
    zb.row({}).row({}).row({});
    expect(run<double>(za, eb).rp == std::vector<int64_t>({0, 0, 0}), "nnz(A) = 0");
    expect(run<double>(ea, zb).rp == std::vector<int64_t>({0, 0, 0, 0}), "nnz(B) = 0");
    expect(run<double>(Csr(3), eb).rp == std::vector<int64_t>({0}), "m = 0");
    Csr k0(0);
    k0.row({}).row({});
    expect(run<float>(k0, Csr(4)).rp == std::vector<int64_t>({0, 0, 0}), "k = 0");
    Csr n0(0);
    n0.row({}).row({}).row({});
    expect(run<double>(ea, n0).rp == std::vector<int64_t>({0, 0, 0, 0}), "n = 0");
    // the errors
    Csr u(4);
    u.row({{0, 1.0}}).row({{2, 1.0}, {1, 1.0}}).row({{3, 1.0}, {3, 1.0}});
    o = run<double>(ea, u);
    expect(o.rc == CVR_ERR_INVALID && o.bad == 1, "B out of order");
    Csr u2(4);
    u2.row({{0, 1.0}}).row({{1, 1.0}}).row({{3, 1.0}, {3, 1.0}});
    o = run<double>(ea, u2);
    expect(o.rc == CVR_ERR_INVALID && o.bad == 2, "B with a duplicate");
    o = run<double>(a, eb);
    expect(o.rc == CVR_ERR_INVALID && o.bad == -1, "the inner dimensions differ");
    Csr oc(2);
    oc.row({{2, 1.0}}).row({});
    expect(run<double>(oc, b).rc == CVR_ERR_INVALID, "a column of A outside the matrix");
    {
        cvr_csr_view va{}, vb{};
        int64_t      rp[2] = {0, 0}, bad = 0, crp[2];
        int32_t      ci[1];
        va.nrows = va.ncols = vb.nrows = vb.ncols = 1;
        va.row_ptr = vb.row_ptr = rp;
        expect(cvr_spgemm_host(nullptr, &vb, crp, nullptr, nullptr, &bad) == CVR_ERR_INVALID, "null A");
        expect(cvr_spgemm_host(&va, nullptr, crp, nullptr, nullptr, &bad) == CVR_ERR_INVALID, "null B");
        expect(cvr_spgemm_host(&va, &vb, nullptr, nullptr, nullptr, &bad) == CVR_ERR_INVALID, "null row_ptr");
        expect(cvr_spgemm_host(&va, &vb, crp, nullptr, nullptr, nullptr) == CVR_ERR_INVALID, "null bad_row");
        expect(cvr_spgemm_host(&va, &vb, crp, ci, nullptr, &bad) == CVR_ERR_INVALID, "col_idx without vals");
        vb.is_f32 = 1;
        expect(cvr_spgemm_host(&va, &vb, crp, nullptr, nullptr, &bad) == CVR_ERR_INVALID, "is_f32 differs");
        vb.is_f32 = 0;
        vb.arrays_on_device = 1;
        expect(cvr_spgemm_host(&va, &vb, crp, nullptr, nullptr, &bad) == CVR_ERR_INVALID, "device arrays");
        vb.arrays_on_device = 0;
        vb.ncols = 0x7fffffff;
        expect(cvr_spgemm_host(&va, &vb, crp, nullptr, nullptr, &bad) == CVR_ERR_INVALID, "ncols of B at 2^31 - 1");
        vb.ncols = 1;
        expect(cvr_spgemm_host(&va, &vb, crp, nullptr, nullptr, &bad) == CVR_OK && crp[1] == 0 && bad == -1, "1 x 1 without entries");
    }
    if (failures) return 1;
    printf("spgemm_host_check: all cases ran clean\n");
    return 0;
}
