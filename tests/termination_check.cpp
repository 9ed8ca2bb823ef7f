// check_termination of enlsip.jl_amd/csrc/gn_batch_records.hpp and the placing of TerminationScratch on the CPU: every numbered
// argument error of enlsip_gn_termination_batched_dev in the order the header documents, the lower problem index winning, and
// problems that are not taken left unread.  A stand-alone program (tests/test_termination_host.py builds it, with the host
// sanitizers where they are available); it prints one line per assertion and returns the number that failed.
#include <cstdio>
#include <string>
#include <vector>

#include "../enlsip.jl_amd/csrc/gn_batch_records.hpp"

using namespace gn;

static int failed = 0;
static void expect(bool ok, const char* name) {
    std::printf("%s %s\n", ok ? "ok" : "FAILED", name);
    failed += !ok;
}

int main() {
    const int64_t B = 3, m = 9, n = 4, l = 5, t_max = 3;
    std::vector<enlsip_gn_term_state> st(B);
    std::vector<int64_t> act(B * l, 0), ina(B * l, 0), take(B, 1);
    for (int64_t k = 0; k < B; ++k) {
        st[k] = {};
        st[k].t = 2; st[k].q = 1; st[k].l = l; st[k].dimJ2 = n;
        act[k * l] = 1; act[k * l + 1] = 3;
        ina[k * l] = 2; ina[k * l + 1] = 4; ina[k * l + 2] = 5;
    }
    const TerminationShape good{B, m, n, l, t_max, m, m * n, n, n * t_max};
    std::string err;
    auto run = [&](TerminationShape s, bool host = true, bool dm = true, bool dl = true, bool dt = true, bool dn = true,
                   const int64_t* a = nullptr, const int64_t* i = nullptr, const enlsip_gn_term_state* state = nullptr) {
        err.clear();
        return check_termination(err, s, state ? state : st.data(), a ? a : act.data(), i ? i : ina.data(), take.data(), host, dm, dl, dt, dn);
    };
    expect(run(good) == 0 && err.empty(), "a good call passes");
    { auto s = good; s.batch = 0; expect(run(s) == -2, "-2 batch < 1"); }
    { auto s = good; s.m = -1; expect(run(s) == -3, "-3 m < 0"); }
    { auto s = good; s.n = 0; expect(run(s) == -3, "-3 n < 1"); }
    { auto s = good; s.l = 1025; s.t_max = 3; expect(run(s) == -3, "-3 l > 1024"); }
    { auto s = good; s.t_max = l + 1; expect(run(s) == -3, "-3 t_max > l"); }
    expect(run(good, false) == -4, "-4 tol, sums or exit_code NULL");
    expect(run(good, true, false) == -4, "-4 dJ or drx NULL while m > 0");
    { auto s = good; s.m = 0; s.ldj = 1; s.strideJ = n; expect(run(s, true, false) == 0, "dJ and drx may be NULL when m == 0"); }
    expect(run(good, true, true, false) == -4, "-4 dcx_all or dw NULL while l > 0");
    expect(run(good, true, true, true, false) == -4, "-4 a slot pointer NULL while t_max > 0");
    expect(run(good, true, true, true, true, false) == -4, "-4 an n-vector NULL");
    {
        err.clear();
        const int rc = check_termination(err, good, nullptr, act.data(), ina.data(), take.data(), true, true, true, true, true);
        expect(rc == -4, "-4 state NULL");
        err.clear();
        const int rc2 = check_termination(err, good, st.data(), nullptr, ina.data(), take.data(), true, true, true, true, true);
        expect(rc2 == -4, "-4 active NULL while l > 0");
        err.clear();
        const int rc3 = check_termination(err, good, st.data(), act.data(), nullptr, take.data(), true, true, true, true, true);
        expect(rc3 == -4, "-4 inactive NULL while l > 0");
    }
    { auto s2 = st; s2[1].t = t_max + 1; expect(run(good, true, true, true, true, true, nullptr, nullptr, s2.data()) == -5 && err.find("[1]") != std::string::npos, "-5 t outside 0..t_max names k"); }
    { auto s2 = st; s2[2].l = l - 1; expect(run(good, true, true, true, true, true, nullptr, nullptr, s2.data()) == -5 && err.find("[2]") != std::string::npos, "-5 state.l != l names k"); }
    { auto s2 = st; s2[0].q = 3; expect(run(good, true, true, true, true, true, nullptr, nullptr, s2.data()) == -6 && err.find("[0]") != std::string::npos, "-6 q outside 0..t names k"); }
    { auto a2 = act; a2[1 * l + 1] = l + 1; expect(run(good, true, true, true, true, true, a2.data()) == -7 && err.find("active[1][1]") != std::string::npos, "-7 an active entry outside 0..l"); }
    { auto i2 = ina; i2[2 * l + 2] = -1; expect(run(good, true, true, true, true, true, nullptr, i2.data()) == -7 && err.find("inactive[2][2]") != std::string::npos, "-7 an inactive entry outside 0..l"); }
    { auto i2 = ina; i2[2 * l + 3] = 99; expect(run(good, true, true, true, true, true, nullptr, i2.data()) == 0, "entries behind the used part are not read"); }
    { auto s2 = st; s2[1].dimJ2 = n + 1; expect(run(good, true, true, true, true, true, nullptr, nullptr, s2.data()) == -8, "-8 dimJ2 outside 0..n"); }
    { auto s2 = st; s2[1].t = 9; s2[2].q = 9; expect(run(good, true, true, true, true, true, nullptr, nullptr, s2.data()) == -5 && err.find("[1]") != std::string::npos, "the lower k wins"); }
    { auto s2 = st; s2[1].t = 9; take[1] = 0; expect(run(good, true, true, true, true, true, nullptr, nullptr, s2.data()) == 0, "a problem that is not taken is not checked"); take[1] = 1; }
    { auto s = good; s.ldj = m - 1; expect(run(s) == -9, "-9 ldj < m"); }
    { auto s = good; s.ldat = n - 1; expect(run(s) == -9, "-9 ldat < n"); }
    { auto s = good; s.strideJ = m * n - 1; expect(run(s) == -10, "-10 strideJ < ldj * n"); }
    { auto s = good; s.strideAt = n * t_max - 1; expect(run(s) == -10, "-10 strideAt < ldat * t_max"); }
    { auto s2 = st; s2[0].t = 9; auto s = good; s.ldj = 1; expect(run(s, true, true, true, true, true, nullptr, nullptr, s2.data()) == -5, "a per-problem error comes before the leading dimensions"); }
    // the layout: the moved arrays at equal offsets with and without the partial sums, the sums record as the header declares it
    const size_t with = layout_bytes<TerminationScratch>(B, 2 * l, (int64_t)7), without = layout_bytes<TerminationScratch>(B, 2 * l, (int64_t)0);
    expect(with == without + (size_t)B * 7 * sizeof(double), "the partial sums come last");
    std::vector<char> buf(with);
    TerminationScratch S;
    Carver c;
    c.base = buf.data();
    S.carve(c, B, 2 * l, 7);
    expect(S.up_bytes == (size_t)B * sizeof(TermMeta) + (size_t)B * 2 * l * sizeof(int) && S.down_bytes == (size_t)B * sizeof(enlsip_gn_term_sums),
           "one copy up [meta | lists], one copy down [sums]");
    expect(sizeof(TermMeta) == 24 && sizeof(enlsip_gn_term_sums) == 120, "record sizes");
    return failed;
}
