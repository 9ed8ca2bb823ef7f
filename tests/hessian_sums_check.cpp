// The host side of the batched Hessian sums on the CPU: check_hessian_points, check_hessian_sums and HessianScratch of
// enlsip.jl_amd/csrc/gn_batch_records.hpp (every argument error of enlsip_gn_hessian_points_batched_dev and
// enlsip_gn_hessian_sums_batched_dev, the lower problem index winning, problems with a negative slot left unread), the pair decode
// of gn_hessian_sums.hpp for every pair of n = 1..64 and for the last pairs of n = 46341 (where the pair index first passes 2^30),
// and hess_points / hess_sums on buffers of exactly their used size with pair ranges at both ends of the index.  A stand-alone
// program (tests/test_hessian_sums_host.py builds it with the host sanitizers where no GPU is present); it prints one line per
// assertion and returns the number that failed.
#include <cstdio>
#include <string>
#include <vector>

#include "../enlsip.jl_amd/csrc/gn_batch_records.hpp"
#include "../enlsip.jl_amd/csrc/gn_hessian_sums.hpp"

using namespace gn;

static int failed = 0;
static void expect(bool ok, const char* name) {
    std::printf("%s %s\n", ok ? "ok" : "FAILED", name);
    failed += !ok;
}

int main() {
    std::string err;
    // ---- the points call ----------------------------------------------------------------------------------------------------------
    auto pts = [&](int64_t count, int64_t n, int64_t pair0, int64_t npairs, bool x = true, bool X = true) {
        err.clear();
        return check_hessian_points(err, count, n, pair0, npairs, x, X);
    };
    expect(pts(3, 4, 0, 10) == 0 && err.empty(), "points: a good call passes");
    expect(pts(0, 4, 0, 10) == -2, "points: -2 count < 1");
    expect(pts(3, 0, 0, 1) == -2, "points: -2 n < 1");
    expect(pts(3, 4, 0, 0) == -2, "points: -2 npairs < 1");
    expect(pts(3, 4, -1, 2) == -2, "points: -2 pair0 < 0");
    expect(pts(3, 4, 1, 10) == -2, "points: -2 pair0 + npairs > n (n + 1) / 2");
    expect(pts(3, 4, 10, 1) == -2, "points: -2 pair0 at the end of the triangle");
    expect(pts(3, 4, 9, 1) == 0, "points: the last pair alone");
    expect(pts(3, 4, 0, INT64_MAX) == -2, "points: -2 npairs beyond every triangle, no overflow");
    expect(pts(1 << 20, 1 << 20, 0, 1LL << 30) == -2, "points: -2 a buffer beyond 2^48 doubles");
    expect(pts(3, 4, 0, 10, false) == -4, "points: -4 x NULL");
    expect(pts(3, 4, 0, 10, true, false) == -4, "points: -4 X NULL");

    // ---- the sums call ------------------------------------------------------------------------------------------------------------
    const int64_t B = 3, m = 9, n = 4, l = 5, t_max = 3;
    std::vector<int64_t> t{2, 0, 3}, act(B * l, 0), slot{2, 0, 1};
    act[0] = 1; act[1] = 5; act[2 * l] = 4; act[2 * l + 1] = 0; act[2 * l + 2] = 2;
    const HessianShape good{B, m, n, l, t_max, 0, 10, n, n * n};
    struct Ptrs { bool x = true, F = true, rx = true, G = true, lambda = true, Gamma = true; };
    auto run = [&](HessianShape s, Ptrs p = Ptrs(), const int64_t* tt = nullptr, const int64_t* a = nullptr, const int64_t* sl = nullptr,
                   bool no_t = false, bool no_act = false) {
        err.clear();
        return check_hessian_sums(err, s, no_t ? nullptr : (tt ? tt : t.data()), no_act ? nullptr : (a ? a : act.data()), sl, p.x, p.F,
                                  p.rx, p.G, p.lambda, p.Gamma);
    };
    expect(run(good) == 0 && err.empty(), "sums: a good call passes");
    expect(run(good, Ptrs(), nullptr, nullptr, slot.data()) == 0, "sums: a permuted slot passes");
    { auto s = good; s.count = 0; expect(run(s) == -2, "sums: -2 count < 1"); }
    { auto s = good; s.n = 0; expect(run(s) == -2, "sums: -2 n < 1"); }
    { auto s = good; s.m = -1; expect(run(s) == -2, "sums: -2 m < 0"); }
    { auto s = good; s.l = -1; expect(run(s) == -2, "sums: -2 l < 0"); }
    { auto s = good; s.t_max = -1; expect(run(s) == -2, "sums: -2 t_max < 0"); }
    { auto s = good; s.npairs = 0; expect(run(s) == -2, "sums: -2 npairs < 1"); }
    { auto s = good; s.pair0 = -1; expect(run(s) == -2, "sums: -2 pair0 < 0"); }
    { auto s = good; s.pair0 = 1; expect(run(s) == -2, "sums: -2 pair0 + npairs > n (n + 1) / 2"); }
    { auto s = good; s.pair0 = 9; s.npairs = 1; expect(run(s) == 0, "sums: the last pair alone"); }
    { auto s = good; s.pair0 = 10; s.npairs = 1; expect(run(s) == -2, "sums: -2 one pair past the end"); }
    expect(run(good, Ptrs(), nullptr, nullptr, nullptr, true) == -4, "sums: -4 t NULL");
    { Ptrs p; p.x = false; expect(run(good, p) == -4, "sums: -4 dx NULL"); }
    { Ptrs p; p.Gamma = false; expect(run(good, p) == -4, "sums: -4 dGamma NULL"); }
    { Ptrs p; p.F = false; expect(run(good, p) == -4, "sums: -4 dF NULL while m > 0"); }
    { Ptrs p; p.rx = false; expect(run(good, p) == -4, "sums: -4 drx NULL while m > 0"); }
    { Ptrs p; p.F = false; p.rx = false; auto s = good; s.m = 0; expect(run(s, p) == 0, "sums: dF and drx may be NULL when m == 0"); }
    { Ptrs p; p.G = false; expect(run(good, p) == -4, "sums: -4 dG NULL while some t[k] > 0"); }
    { Ptrs p; p.lambda = false; expect(run(good, p) == -4, "sums: -4 dlambda NULL while some t[k] > 0"); }
    expect(run(good, Ptrs(), nullptr, nullptr, nullptr, false, true) == -4, "sums: -4 active NULL while some t[k] > 0");
    {
        Ptrs p; p.G = false; p.lambda = false;
        std::vector<int64_t> t0{0, 0, 0};
        expect(run(good, p, t0.data(), nullptr, nullptr, false, true) == 0, "sums: the constraint side may be NULL when every t[k] == 0");
        auto s = good; s.l = 0; s.t_max = 0;
        expect(run(s, p, t0.data(), nullptr, nullptr, false, true) == 0, "sums: l == 0 needs no constraint side");
        std::vector<int64_t> sl{-1, 0, -1};
        expect(run(good, p, nullptr, nullptr, sl.data(), false, true) == 0, "sums: only problems with a slot count for the pointers");
    }
    { auto t2 = t; t2[1] = t_max + 1; expect(run(good, Ptrs(), t2.data()) == -5 && err.find("t[1]") != std::string::npos, "sums: -5 t outside 0..t_max names k"); }
    { auto t2 = t; t2[0] = -1; expect(run(good, Ptrs(), t2.data()) == -5, "sums: -5 t < 0"); }
    { auto s = good; s.l = 2; s.t_max = 3; auto t2 = t; t2[0] = 0; expect(run(s, Ptrs(), t2.data()) == -5 && err.find("t[2]") != std::string::npos, "sums: -5 t above l"); }
    { auto a2 = act; a2[1] = l + 1; expect(run(good, Ptrs(), nullptr, a2.data()) == -5 && err.find("active[0][1]") != std::string::npos, "sums: -5 an active entry above l"); }
    { auto a2 = act; a2[2 * l + 2] = -1; expect(run(good, Ptrs(), nullptr, a2.data()) == -5 && err.find("active[2][2]") != std::string::npos, "sums: -5 a negative active entry"); }
    { auto a2 = act; a2[2 * l + 3] = 99; a2[1 * l] = 99; expect(run(good, Ptrs(), nullptr, a2.data()) == 0, "sums: entries behind the used part are not read"); }
    { auto s = good; s.ldg = n - 1; expect(run(s) == -5, "sums: -5 ldg < n"); }
    { auto s = good; s.ldg = n + 2; expect(run(s) == -5, "sums: -5 strideG < ldg * n"); }
    { auto s = good; s.ldg = n + 2; s.strideG = (n + 2) * n + 3; expect(run(s) == 0, "sums: ldg > n and a stride gap pass"); }
    { auto s = good; s.ldg = INT64_MAX; s.strideG = INT64_MAX; expect(run(s) == -5, "sums: -5 ldg * n beyond int64, no overflow"); }
    { std::vector<int64_t> sl{1, 0, 1}; expect(run(good, Ptrs(), nullptr, nullptr, sl.data()) == -5, "sums: -5 two problems share a slot"); }
    { std::vector<int64_t> sl{-1, 7, -1}; expect(run(good, Ptrs(), nullptr, nullptr, sl.data()) == 0, "sums: negative slots may repeat"); }
    { std::vector<int64_t> sl{0, 1LL << 31, 1}; expect(run(good, Ptrs(), nullptr, nullptr, sl.data()) == -5, "sums: -5 a slot beyond 2^31 - 1"); }
    { auto t2 = t; t2[0] = 9; t2[2] = 9; expect(run(good, Ptrs(), t2.data()) == -5 && err.find("[0]") != std::string::npos, "sums: the lower k wins"); }
    { auto t2 = t; t2[0] = 9; std::vector<int64_t> sl{-1, 0, 1}; expect(run(good, Ptrs(), t2.data(), nullptr, sl.data()) == 0, "sums: a problem with a negative slot is not checked"); }
    // the layout: one copy up [meta | active], nothing down
    {
        std::vector<char> buf(layout_bytes<HessianScratch>(B, l, (int64_t)0));
        HessianScratch S;
        Carver c;
        c.base = buf.data();
        S.carve(c, B, l, 0);
        expect(S.up_bytes == (size_t)B * sizeof(HessMeta) + (size_t)B * l * sizeof(int) && S.up_bytes == buf.size(), "one copy up [meta | active]");
        expect(sizeof(HessMeta) == 8, "record size");
    }

    // ---- the pair decode ----------------------------------------------------------------------------------------------------------
    {
        bool ok = true;
        for (long long nn = 1; nn <= 64; ++nn) {
            long long P = 0;
            for (long long k = 0; k < nn; ++k)
                for (long long j = 0; j <= k; ++j, ++P) {
                    long long kk = -1, jj = -1;
                    hess_decode(P, &kk, &jj);
                    ok = ok && kk == k && jj == j;
                }
            ok = ok && P == hess_pairs(nn);
        }
        expect(ok, "decode: every pair of n = 1..64 in the reference's loop order");
        const long long nn = 46341;      // the first n whose pair count passes 2^30 (and whose n * n passes 2^31)
        ok = hess_pairs(nn) == 1073767311LL && hess_pairs(nn) > (1LL << 30) && hess_pairs(nn - 1) < (1LL << 30) && nn * nn > (1LL << 31);
        for (long long k = nn - 3; k < nn; ++k)
            for (long long j : {0LL, 1LL, k / 2, k - 1, k}) {
                long long kk = -1, jj = -1;
                hess_decode(k * (k + 1) / 2 + j, &kk, &jj);
                ok = ok && kk == k && jj == j;
            }
        expect(ok, "decode: the last rows of n = 46341, first and last pair of each");
        long long kk, jj;
        hess_decode((1LL << 61) - 1, &kk, &jj);
        expect(kk * (kk + 1) / 2 + jj == (1LL << 61) - 1 && jj >= 0 && jj <= kk, "decode: a pair index near 2^61");
    }

    // ---- the routines on buffers of exactly their used size (the sanitizers see a read or write past an end) ----------------------
    {
        const double e1 = hess_eps1();
        expect(e1 > 6.0554544e-6 && e1 < 6.0554545e-6, "eps1 = eps^(1/3)");
        const long long nn = 3, pairs = hess_pairs(nn);
        std::vector<double> x{0.5, -3.0, 0.0};
        const double e0 = e1, ex1 = 3.0 * e1;
        {   // both ends of the index, one pair each
            std::vector<double> X(4 * nn);
            hess_points(nn, 0, 1, x.data(), e1, X.data());
            expect(X[0] == (0.5 + e0) + e0 && X[3] == (0.5 - e0) + e0 && X[6] == (0.5 + e0) - e0 && X[9] == (0.5 - e0) - e0 && X[1] == -3.0 && X[2] == 0.0,
                   "points: the first pair is the diagonal (0, 0), two roundings of one entry");
            hess_points(nn, pairs - 1, 1, x.data(), e1, X.data());
            expect(X[2] == (0.0 + e0) + e0 && X[5] == (0.0 - e0) + e0 && X[0] == 0.5 && X[1] == -3.0, "points: the last pair is the diagonal (n - 1, n - 1)");
            hess_points(nn, 1, 1, x.data(), e1, X.data());      // (k, j) = (1, 0)
            expect(X[0] == 0.5 + e0 && X[1] == -3.0 + ex1 && X[3] == 0.5 - e0 && X[4] == -3.0 + ex1 && X[6] == 0.5 + e0 && X[7] == -3.0 - ex1 &&
                       X[9] == 0.5 - e0 && X[10] == -3.0 - ex1, "points: signs (+,+), (-,+), (+,-), (-,-) in the order (j, k)");
        }
        const long long mm = 70, ll = 3, tt = 2;
        std::vector<int64_t> a{3, 0};
        std::vector<double> rx(mm, 1.0), lam{2.0, 5.0};
        for (long long pair0 : {0LL, 2LL, pairs - 1}) {
            const long long np = pair0 == 2 ? 3 : 1;
            std::vector<double> F(np * 4 * mm, 0.0), G(np * 4 * ll, 0.0), Gam(nn * nn, -1.0);
            for (long long q = 0; q < np; ++q) {
                for (long long i = 0; i < mm; ++i) F[(q * 4 + 0) * mm + i] = 1.0;      // f1 - f2 - f3 + f4 = 1 per row: s_r = m
                G[(q * 4 + 3) * ll + 2] = 0.5;                                          // g4[active 3] = 0.5: s_c = 0.5 * 2 = 1
            }
            hess_sums({mm, nn, ll, tt, pair0, np, a.data(), x.data(), F.data(), rx.data(), G.data(), lam.data()}, e1, Gam.data(), nn);
            bool ok = true;
            int written = 0;
            for (long long q = 0; q < np; ++q) {
                long long k, j;
                hess_decode(pair0 + q, &k, &j);
                const double ek = hess_eps(x[k], e1), ej = hess_eps(x[j], e1);
                const double want = 70.0 / ((4 * ej) * ek) - 1.0 / ((4.0 * ek) * ej);
                ok = ok && Gam[k + j * nn] == want && Gam[j + k * nn] == want;
            }
            for (double v : Gam) written += v != -1.0;
            ok = ok && written == (pair0 == 2 ? 5 : 1);      // pairs 2, 3, 4 = (1, 1), (2, 0), (2, 1): 1 + 2 + 2 entries
            expect(ok, pair0 == 0 ? "sums: the first pair, exact buffers" : pair0 == 2 ? "sums: a range inside the index, only its entries written"
                                                                                       : "sums: the last pair, exact buffers");
        }
        {   // m == 0 and t == 0: no array is read
            std::vector<double> Gam(nn * nn, -1.0);
            hess_sums({0, nn, 0, 0, 0, pairs, nullptr, x.data(), nullptr, nullptr, nullptr, nullptr}, e1, Gam.data(), nn);
            bool ok = true;
            for (double v : Gam) ok = ok && v == 0.0;
            expect(ok, "sums: m == 0 and t == 0 give a zero Gamma from no array");
        }
        expect(hess_eps(NAN, e1) != hess_eps(NAN, e1) && hess_eps(-0.0, e1) == e1 && hess_eps(-2.0, e1) == 2.0 * e1, "eps_k = max(|x|, 1.0) eps1, a NaN stays a NaN");
    }
    return failed;
}
