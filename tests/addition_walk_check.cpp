// Runs the host side of the batched working-set additions on the CPU for tests/test_addition_walk_san.py: the walk and the rebuild
// (csrc/gn_violated_constraints.hpp) at their edges, the new records, the checks and the scratch layout
// (csrc/gn_batch_records.hpp).  One line per named assertion, "ok <name>" or "FAIL <name> ..."; the exit status is the number of
// failures.  Every buffer has exactly its used size, so that the sanitizers see a read or a write that leaves it.
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "../enlsip.jl_amd/csrc/gn_batch_records.hpp"
#include "../enlsip.jl_amd/csrc/gn_violated_constraints.hpp"

using namespace gn;
using I = int64_t;

static int failures = 0;
static bool all_of_group = true;
#define EXPECT(cond) \
    do { if (!(cond)) { all_of_group = false; printf("  failed at line %d: %s\n", __LINE__, #cond); } } while (0)
static void group(const char* name) {
    printf("%s %s\n", all_of_group ? "ok" : "FAIL", name);
    failures += !all_of_group;
    all_of_group = true;
}

struct Walk {
    long long t;
    std::vector<I> act, ina;
    int added, status;
};
// heap buffers of exactly l entries each
static Walk walk(long long l, long long n, long long q, long long t, std::vector<I> act, std::vector<I> ina, std::vector<double> cx,
                 long long iau) {
    std::unique_ptr<I[]> a(new I[l]), i(new I[l]);
    std::unique_ptr<double[]> c(new double[l]);
    for (long long j = 0; j < l; ++j) { a[j] = act[j]; i[j] = ina[j]; c[j] = cx[j]; }
    Walk w;
    w.t = t;
    w.status = addition_walk<I>(l, n, q, &w.t, a.get(), i.get(), c.get(), iau, &w.added);
    w.act.assign(a.get(), a.get() + l);
    w.ina.assign(i.get(), i.get() + l);
    return w;
}
static bool is(const std::vector<I>& v, std::initializer_list<I> want) { return v == std::vector<I>(want); }

static void walks() {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    Walk w = walk(1, 1, 0, 0, {0}, {1}, {-1.0}, 0);
    EXPECT(w.t == 1 && w.added == 1 && w.status == 0 && is(w.act, {1}) && is(w.ina, {0}));
    w = walk(1, 1, 0, 0, {0}, {1}, {1.0}, 0);
    EXPECT(w.t == 0 && w.added == 0 && w.status == 0 && is(w.act, {0}) && is(w.ina, {1}));
    w = walk(1, 1, 0, 1, {1}, {0}, {-1.0}, 1);
    EXPECT(w.t == 1 && w.added == 0 && w.status == 0 && is(w.act, {1}));
    group("walk_l_1");
    w = walk(3, 3, 3, 3, {1, 2, 3}, {0, 0, 0}, {-1.0, -1.0, -1.0}, 2);
    EXPECT(w.t == 3 && w.added == 0 && w.status == 0 && is(w.act, {1, 2, 3}) && is(w.ina, {0, 0, 0}));
    group("walk_q_equals_l_full_active_list");
    w = walk(4, 7, 0, 0, {0, 0, 0, 0}, {1, 2, 3, 4}, {-1.0, -2.0, -3.0, -4.0}, 0);
    EXPECT(w.t == 4 && w.added == 1 && w.status == 0 && is(w.act, {1, 2, 3, 4}) && is(w.ina, {0, 0, 0, 0}));
    w = walk(4, 7, 0, 0, {0, 0, 0, 0}, {1, 2, 3, 4}, {nan, 1.0, nan, 0.05}, 4);
    EXPECT(w.t == 1 && w.added == 1 && w.status == 0 && is(w.act, {4, 0, 0, 0}) && is(w.ina, {1, 2, 3, 0}));
    group("walk_empty_active_list_fills_up");
    // capacity 1: the removed constraint 3 sorts behind the candidate 1, a true swap into the last slot of the inactive list
    w = walk(3, 1, 0, 1, {3, 0, 0}, {1, 2, 0}, {-1.0, 3.0, 0.5}, 0);
    EXPECT(w.t == 1 && w.added == 1 && w.status == 0 && is(w.act, {1, 0, 0}) && is(w.ina, {2, 3, 0}));
    // capacity 2 with a tie: the first maximum leaves
    w = walk(5, 2, 0, 2, {4, 5, 0, 0, 0}, {1, 2, 3, 0, 0}, {1.0, 2.0, -3.0, 0.5, 0.5}, 0);
    EXPECT(w.t == 2 && w.added == 1 && w.status == 0 && is(w.act, {3, 5, 0, 0, 0}) && is(w.ina, {1, 2, 4, 0, 0}));
    // the equalities are no candidates: nothing to swap out
    w = walk(3, 1, 1, 1, {1, 0, 0}, {2, 3, 0}, {5.0, -1.0, -2.0}, 0);
    EXPECT(w.t == 1 && w.added == 0 && w.status == 0 && is(w.act, {1, 0, 0}) && is(w.ina, {2, 3, 0}));
    group("walk_capacity_swaps");
    // the removed constraint would come straight back: stopped with the lists untouched
    w = walk(3, 1, 0, 1, {1, 0, 0}, {2, 3, 0}, {0.5, -1.0, 2.0}, 0);
    EXPECT(w.t == 1 && w.added == 0 && w.status == 1 && is(w.act, {1, 0, 0}) && is(w.ina, {2, 3, 0}));
    // ... after an earlier pass that added (the quirk of :642 puts 2 in, not the violated 3)
    w = walk(4, 1, 0, 1, {1, 0, 0, 0}, {2, 3, 4, 0}, {0.5, 1.0, -1.0, 2.0}, 0);
    EXPECT(w.t == 1 && w.added == 1 && w.status == 1 && is(w.act, {2, 0, 0, 0}) && is(w.ina, {1, 3, 4, 0}));
    group("walk_status_1_leaves_the_lists");
    // padding zeros inside the used part are skipped, never dereferenced
    w = walk(3, 3, 0, 1, {0, 0, 0}, {0, 2, 0}, {-1.0, -1.0, -1.0}, 0);
    EXPECT(w.status == 0 && w.t == 2 && w.added == 1);
    group("walk_zero_entries");
}

static void gathers() {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    {   // l = 1, n = 1
        std::unique_ptr<double[]> A(new double[1]{-3.0}), cx(new double[1]{6.0}), At(new double[1]{nan}), ca(new double[1]), ds(new double[1]);
        std::unique_ptr<I[]> act(new I[1]{1});
        gather_active<I>(1, 1, act.get(), A.get(), 1, cx.get(), true, At.get(), 1, ca.get(), ds.get());
        EXPECT(At[0] == -1.0 && ca[0] == 2.0 && ds[0] == 1.0 / 3.0);
        gather_active<I>(1, 1, act.get(), A.get(), 1, cx.get(), false, At.get(), 1, ca.get(), ds.get());
        EXPECT(At[0] == -3.0 && ca[0] == 6.0 && ds[0] == 3.0);
        gather_active<I>(1, 0, act.get(), A.get(), 1, cx.get(), true, nullptr, 1, nullptr, nullptr);      // t == 0: nothing is touched
    }
    group("gather_l_1_and_t_0");
    {   // full list, n = 65 (two strided partials in slot 0), lda > l, ldat > n with canaries
        const long long l = 3, n = 65, lda = 5, ldat = 67;
        std::unique_ptr<double[]> A(new double[lda * (n - 1) + l]), cx(new double[l]{1.0, 2.0, 3.0}), At(new double[ldat * (l - 1) + n]),
            ca(new double[l]), ds(new double[l]);
        for (long long j = 0; j < n; ++j)
            for (long long r = 0; r < lda && lda * j + r < lda * (n - 1) + l; ++r) A[lda * j + r] = r < l ? (double)(r + 1) : nan;
        for (long long k = 0; k < ldat * (l - 1) + n; ++k) At[k] = nan;
        std::unique_ptr<I[]> act(new I[l]{1, 2, 3});
        gather_active<I>(n, l, act.get(), A.get(), lda, cx.get(), false, At.get(), ldat, ca.get(), ds.get());
        bool ok = true;
        for (long long c = 0; c < l; ++c) {
            for (long long j = 0; j < n; ++j) ok = ok && At[c * ldat + j] == (double)(c + 1);
            for (long long j = n; j < ldat && c * ldat + j < ldat * (l - 1) + n; ++j) ok = ok && std::isnan(At[c * ldat + j]);
            ok = ok && ds[c] == std::sqrt(65.0 * (double)((c + 1) * (c + 1))) && ca[c] == (double)(c + 1);
        }
        EXPECT(ok);
        gather_active<I>(n, l, act.get(), A.get(), lda, cx.get(), true, At.get(), ldat, ca.get(), ds.get());
        ok = true;
        for (long long c = 0; c < l; ++c) {
            const double div = std::sqrt(65.0 * (double)((c + 1) * (c + 1)));
            for (long long j = 0; j < n; ++j) ok = ok && At[c * ldat + j] == (double)(c + 1) / div;
            ok = ok && ds[c] == 1.0 / div && ca[c] == (double)(c + 1) / div;
        }
        EXPECT(ok);
    }
    group("gather_full_list_padded_leading_dimensions");
    {   // a zero row and an entry 0 of the list
        const long long l = 2, n = 3;
        std::unique_ptr<double[]> A(new double[l * n]{0.0, 1.0, 0.0, 2.0, 0.0, 2.0}), cx(new double[l]{4.0, 9.0}), At(new double[n * 2]),
            ca(new double[2]), ds(new double[2]);
        std::unique_ptr<I[]> act(new I[2]{1, 0});
        gather_active<I>(n, 2, act.get(), A.get(), l, cx.get(), true, At.get(), n, ca.get(), ds.get());
        EXPECT(ds[0] == 1.0 && ds[1] == 1.0 && ca[0] == 4.0 && ca[1] == 0.0 && At[0] == 0.0 && At[3] == 0.0 && At[5] == 0.0);
        gather_active<I>(n, 2, act.get(), A.get(), l, cx.get(), false, At.get(), n, ca.get(), ds.get());
        EXPECT(ds[0] == 0.0 && ds[1] == 0.0);
        act[1] = 2;
        gather_active<I>(n, 2, act.get(), A.get(), l, cx.get(), true, At.get(), n, ca.get(), ds.get());
        EXPECT(ds[1] == 1.0 / 3.0 && At[3] == 1.0 / 3.0 && At[4] == 2.0 / 3.0 && ca[1] == 3.0);
    }
    group("gather_zero_row_and_zero_entry");
}

static void records_and_layout() {
    EXPECT(sizeof(AdditionMeta) == 16 && offsetof(AdditionMeta, t) == 0 && offsetof(AdditionMeta, q) == 4 &&
           offsetof(AdditionMeta, take) == 8 && offsetof(AdditionMeta, index_alpha_upp) == 12);
    group("record_AdditionMeta");
    EXPECT(sizeof(AdditionOut) == 16 && offsetof(AdditionOut, t) == 0 && offsetof(AdditionOut, added) == 4 &&
           offsetof(AdditionOut, status) == 8 && offsetof(AdditionOut, pad) == 12);
    group("record_AdditionOut");
    const int64_t tk[4] = {0, 1, 2, 7};
    EXPECT(addition_take(nullptr, 3) == 1 && addition_take(tk, 0) == 0 && addition_take(tk, 1) == 1 && addition_take(tk, 2) == 2 &&
           addition_take(tk, 3) == 1);
    group("addition_take");
    for (int64_t batch : {1, 5})
        for (int64_t l : {1, 3, 1024}) {
            const size_t bytes = layout_bytes<AdditionScratch>(batch, 2 * l, (int64_t)0);
            std::unique_ptr<char[]> mem(new char[bytes]);
            AdditionScratch S;
            Carver c;
            c.base = mem.get();
            S.carve(c, batch, 2 * l, 0);
            EXPECT((char*)S.meta == mem.get() && (char*)S.list == mem.get() + 16 * batch);
            EXPECT(S.up_bytes == (size_t)(16 * batch + 8 * batch * l));
            EXPECT((char*)S.out == (char*)S.list + 8 * batch * l && addition_down_bytes(S, batch) == (size_t)(8 * batch * l + 16 * batch));
            EXPECT((char*)(S.out + batch) == mem.get() + bytes);      // nothing behind the records: no partial sums
            memset(S.meta, 0, S.up_bytes);
            memset(S.list, 0, addition_down_bytes(S, batch));
        }
    group("layout_addition");
}

static void checks() {
    std::string e;
    const int64_t B = 2, n = 2, l = 3;
    std::unique_ptr<int64_t[]> q(new int64_t[B]{0, 1}), t(new int64_t[B]{2, 1}), act(new int64_t[B * l]{1, 3, 0, 2, 0, 0}),
        ina(new int64_t[B * l]{2, 0, 0, 1, 3, 0}), iau(new int64_t[B]{0, 3});
    AdditionShape s{B, n, l, 2, l, l * n, n, n * 2};
    auto run = [&](const AdditionShape& sh, const int64_t* take = nullptr) {
        return check_addition(e, sh, q.get(), t.get(), act.get(), ina.get(), iau.get(), take, true, true, true);
    };
    EXPECT(run(s) == 0);
    AdditionShape b = s;
    b.batch = 0; EXPECT(run(b) == -2);
    b = s; b.n = 0; EXPECT(run(b) == -3);
    b = s; b.l = 1025; EXPECT(run(b) == -3);
    b = s; b.t_max = 4; EXPECT(run(b) == -3 && e == "t_max > l");
    b = s; b.t_max = 1; EXPECT(run(b) == -5 && e.find("t[0]") != std::string::npos);
    b = s; b.lda = 2; EXPECT(run(b) == -9 && e == "lda < l");
    b = s; b.ldat = 1; EXPECT(run(b) == -9 && e == "ldat < n");
    b = s; b.strideA = 5; EXPECT(run(b) == -10);
    b = s; b.strideAt = 3; EXPECT(run(b) == -10);
    EXPECT(check_addition(e, s, nullptr, t.get(), act.get(), ina.get(), iau.get(), nullptr, true, true, true) == -4);
    EXPECT(check_addition(e, s, q.get(), t.get(), act.get(), ina.get(), iau.get(), nullptr, false, true, true) == -4);
    EXPECT(check_addition(e, s, q.get(), t.get(), act.get(), ina.get(), iau.get(), nullptr, true, false, true) == -4);
    EXPECT(check_addition(e, s, q.get(), t.get(), act.get(), ina.get(), nullptr, nullptr, true, true, true) == 0);
    group("addition_shape_checks");
    q[1] = 2; EXPECT(run(s) == -6 && e == "q[1] outside 0..t[k]"); q[1] = 1;
    act[3] = 4; EXPECT(run(s) == -7 && e == "active[1][0] outside 0..l"); act[3] = 2;
    ina[4] = -1; EXPECT(run(s) == -7 && e == "inactive[1][1] outside 0..l"); ina[4] = 3;
    iau[0] = 4; EXPECT(run(s) == -7 && e == "index_alpha_upp[0] outside 0..l"); iau[0] = 0;
    act[5] = 99; ina[2] = 99; EXPECT(run(s) == 0); act[5] = 0; ina[2] = 0;      // nothing behind the used entries is read
    // n = 3 makes min(l, n) = 3 > t_max = 2: a walk could outgrow the slot, a rebuild cannot
    b = s; b.n = 3; b.strideA = 9; b.ldat = 3; b.strideAt = 6;
    const int64_t only_rebuild[2] = {2, 2}, one_walk[2] = {2, 1}, none[2] = {0, 0};
    EXPECT(run(b) == -5 && run(b, only_rebuild) == 0 && run(b, one_walk) == -5 && e.find("problem 1") != std::string::npos);
    t[0] = -7; EXPECT(run(s) == -5 && run(s, none) == 0); t[0] = 2;      // a problem that is not taken is not checked
    group("addition_per_problem_checks");
}

int main() {
    walks();
    gathers();
    records_and_layout();
    checks();
    printf("%d failures\n", failures);
    return failures;
}
