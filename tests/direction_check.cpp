// The host side of the batched Gauss-Newton direction check on the CPU: check_direction and DirectionScratch of
// enlsip.jl_amd/csrc/gn_batch_records.hpp (every numbered argument error of enlsip_gn_direction_check_batched_dev in the order the
// header documents, the lower problem index winning, problems that are not taken left unread) and dir_sums / dir_status /
// dir_decide of gn_direction_check.hpp on buffers of exactly their used size.  A stand-alone program
// (tests/test_direction_check_host.py builds it with the host sanitizers where no GPU is present); it prints one line per
// assertion and returns the number that failed.
#include <cstdio>
#include <string>
#include <vector>

#include "../enlsip.jl_amd/csrc/gn_batch_records.hpp"
#include "../enlsip.jl_amd/csrc/gn_direction_check.hpp"

using namespace gn;

static int failed = 0;
static void expect(bool ok, const char* name) {
    std::printf("%s %s\n", ok ? "ok" : "FAILED", name);
    failed += !ok;
}

int main() {
    const int64_t B = 3, m = 9, n = 4, l = 5, t_max = 3;
    std::vector<enlsip_gn_dir_state> st(B);
    std::vector<int64_t> act(B * l, 0), ina(B * l, 0), take(B, 1);
    for (int64_t k = 0; k < B; ++k) {
        st[k] = {};
        st[k].t = 2; st[k].q = 1; st[k].l = l; st[k].dimA = 2; st[k].dimJ2 = 2; st[k].rankA = 2;
        act[k * l] = 1; act[k * l + 1] = 3;
        ina[k * l] = 2; ina[k * l + 1] = 4; ina[k * l + 2] = 5;
    }
    const DirectionShape good{B, m, n, l, t_max};
    std::string err;
    auto run = [&](DirectionShape s, bool host = true, bool dm = true, bool dl = true, bool dt = true, const int64_t* a = nullptr,
                   const int64_t* i = nullptr, const enlsip_gn_dir_state* state = nullptr) {
        err.clear();
        return check_direction(err, s, state ? state : st.data(), a ? a : act.data(), i ? i : ina.data(), take.data(), host, dm, dl, dt);
    };
    expect(run(good) == 0 && err.empty(), "a good call passes");
    { auto s = good; s.batch = 0; expect(run(s) == -2, "-2 batch < 1"); }
    { auto s = good; s.m = -1; expect(run(s) == -3, "-3 m < 0"); }
    { auto s = good; s.n = 0; expect(run(s) == -3, "-3 n < 1"); }
    { auto s = good; s.l = 1025; expect(run(s) == -3, "-3 l > 1024"); }
    { auto s = good; s.t_max = l + 1; expect(run(s) == -3, "-3 t_max > l"); }
    expect(run(good, false) == -4, "-4 sums, method_code, beta or status NULL");
    expect(run(good, true, false) == -4, "-4 dd NULL while m > 0");
    { auto s = good; s.m = 0; auto s2 = st; for (auto& x : s2) x.dimJ2 = 0; expect(run(s, true, false, true, true, nullptr, nullptr, s2.data()) == 0, "dd may be NULL when m == 0"); }
    expect(run(good, true, true, false) == -4, "-4 dcx_all NULL while l > 0");
    expect(run(good, true, true, true, false) == -4, "-4 a slot pointer NULL while t_max > 0");
    {
        err.clear();
        expect(check_direction(err, good, nullptr, act.data(), ina.data(), take.data(), true, true, true, true) == -4, "-4 state NULL");
        err.clear();
        expect(check_direction(err, good, st.data(), nullptr, ina.data(), take.data(), true, true, true, true) == -4, "-4 active NULL while l > 0");
        err.clear();
        expect(check_direction(err, good, st.data(), act.data(), nullptr, take.data(), true, true, true, true) == -4, "-4 inactive NULL while l > 0");
    }
    { auto s2 = st; s2[1].t = t_max + 1; expect(run(good, true, true, true, true, nullptr, nullptr, s2.data()) == -5 && err.find("[1]") != std::string::npos, "-5 t outside 0..t_max names k"); }
    { auto s2 = st; s2[2].l = l - 1; expect(run(good, true, true, true, true, nullptr, nullptr, s2.data()) == -5 && err.find("[2]") != std::string::npos, "-5 state.l != l names k"); }
    { auto s2 = st; s2[0].q = 3; expect(run(good, true, true, true, true, nullptr, nullptr, s2.data()) == -6 && err.find("[0]") != std::string::npos, "-6 q outside 0..t names k"); }
    { auto a2 = act; a2[1 * l + 1] = l + 1; expect(run(good, true, true, true, true, a2.data()) == -7 && err.find("active[1][1]") != std::string::npos, "-7 an active entry outside 0..l"); }
    { auto i2 = ina; i2[2 * l + 2] = -1; expect(run(good, true, true, true, true, nullptr, i2.data()) == -7 && err.find("inactive[2][2]") != std::string::npos, "-7 an inactive entry outside 0..l"); }
    { auto i2 = ina; i2[2 * l + 3] = 99; expect(run(good, true, true, true, true, nullptr, i2.data()) == 0, "entries behind the used part are not read"); }
    { auto s2 = st; s2[1].dimA = 3; expect(run(good, true, true, true, true, nullptr, nullptr, s2.data()) == -8 && err.find("dimA[1]") != std::string::npos, "-8 dimA outside 0..t"); }
    { auto s2 = st; s2[1].dimA = -1; expect(run(good, true, true, true, true, nullptr, nullptr, s2.data()) == -8, "-8 dimA < 0"); }
    { auto s2 = st; s2[2].dimJ2 = m + 1; expect(run(good, true, true, true, true, nullptr, nullptr, s2.data()) == -8 && err.find("dimJ2[2]") != std::string::npos, "-8 dimJ2 outside 0..m"); }
    { auto s2 = st; s2[0].prev_t = l + 1; expect(run(good, true, true, true, true, nullptr, nullptr, s2.data()) == -8 && err.find("prev_t[0]") != std::string::npos, "-8 prev_t outside 0..l"); }
    { auto s2 = st; s2[0].prev_dimJ2 = INT64_MAX; expect(run(good, true, true, true, true, nullptr, nullptr, s2.data()) == -8, "-8 prev_dimJ2 beyond 2^31"); }
    { auto s2 = st; s2[0].prev_dimJ2 = INT64_MIN; expect(run(good, true, true, true, true, nullptr, nullptr, s2.data()) == -8, "-8 prev_dimJ2 below -2^31"); }
    { auto s2 = st; s2[0].prev_dimJ2 = -4; expect(run(good, true, true, true, true, nullptr, nullptr, s2.data()) == 0, "a negative prev_dimJ2 (after a Newton step) is legal"); }
    { auto s2 = st; s2[1].t = 9; s2[2].q = 9; expect(run(good, true, true, true, true, nullptr, nullptr, s2.data()) == -5 && err.find("[1]") != std::string::npos, "the lower k wins"); }
    { auto s2 = st; s2[1].t = 9; take[1] = 0; expect(run(good, true, true, true, true, nullptr, nullptr, s2.data()) == 0, "a problem that is not taken is not checked"); take[1] = 1; }
    // the layout: one copy up [meta | lists], one down [sums]; the records as the kernels read them
    std::vector<char> buf(layout_bytes<DirectionScratch>(B, 2 * l, (int64_t)0));
    DirectionScratch S;
    Carver c;
    c.base = buf.data();
    S.carve(c, B, 2 * l, 0);
    expect(S.up_bytes == (size_t)B * sizeof(DirMeta) + (size_t)B * 2 * l * sizeof(int) && S.down_bytes == (size_t)B * sizeof(enlsip_gn_dir_sums),
           "one copy up [meta | lists], one copy down [sums]");
    expect(sizeof(DirMeta) == 24 && sizeof(enlsip_gn_dir_sums) == 64 && sizeof(enlsip_gn_dir_state) == 136, "record sizes");

    // the sums on buffers of exactly their used size (the sanitizers see a read past an end)
    {
        enlsip_gn_dir_state s{};
        s.t = 3; s.q = 1; s.l = 5; s.dimA = 2; s.dimJ2 = 4; s.prev_dimJ2 = 3; s.prev_t = 3; s.rankA = 3;      // k_prev = 2
        std::vector<int64_t> a{2, 0, 5}, i{1, 3};
        std::vector<double> b{3.0, 4.0}, d(70, 1.0), lam{-9.0, -1.0, 2.0}, ds{1.0, 2.0, 4.0}, cx{0.05, 2.0, 0.2, 7.0, 3.0};
        d[64] = 2.0;
        enlsip_gn_dir_sums v{};
        dir_sums(s, {70, 5, a.data(), i.data(), b.data(), d.data(), lam.data(), ds.data(), cx.data(), true}, &v);
        expect(v.b1_sq == 25.0 && v.d_sq == 73.0 && v.d1_sq == 4.0 && v.d1_asprev_sq == 2.0 && v.active_c_sum == 13.0, "sums of a small problem");
        expect(v.n_lm_ge == 1 && v.n_lm_neg == 1 && v.n_inactive_lt_delta == 1, "counts of a small problem");
        expect(dir_status(s, 70, 8) == 0 && dir_status(s, 70, 6) == 2, "status 2: a prefix past n - rankA");
        s.prev_dimJ2 = 72;
        expect(dir_k_prev(s) == 71 && dir_status(s, 70, 8) == 1, "status 1: k_prev > m");
        s.prev_dimJ2 = 71;
        expect(dir_k_prev(s) == 70 && dir_status(s, 70, 80) == 0, "k_prev == m is the whole of d");
        s.prev_dimJ2 = -3;
        dir_sums(s, {70, 5, a.data(), i.data(), b.data(), d.data(), lam.data(), ds.data(), cx.data(), true}, &v);
        expect(v.d1_asprev_sq == 0.0, "k_prev <= 0 is the empty prefix");
        s.t = 0; s.q = 0; s.l = 0; s.dimA = 0; s.dimJ2 = 0;
        dir_sums(s, {0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, false}, &v);
        expect(v.b1_sq == 0.0 && v.d_sq == 0.0 && v.active_c_sum == 0.0 && v.n_lm_ge == 0 && v.n_inactive_lt_delta == 0, "empty problem, no array");
        long long code = 0;
        double beta = -1.0;
        s.iter_number = 0;
        dir_decide(s, v, 0, 4, &code, &beta);
        expect(code == 1 && beta == 0.0, "first iteration: the Gauss-Newton direction");
    }
    return failed;
}
