// Runs the host side of the batched calls on the caller's buffers (csrc/gn_batch_records.hpp) on the CPU for
// tests/test_batch_records_host.py: the record structs, the argument checks, the packing and the scratch layouts.  One line per named
// assertion, "ok <name>" or "FAIL <name> ..."; the exit status is the number of failures.  Every buffer has exactly its used size,
// so that the sanitizers see a read or a write that leaves it.
#include <climits>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <vector>

#include "../enlsip.jl_amd/csrc/gn_batch_records.hpp"

using namespace gn;

static int failures = 0;
static bool all_of_group = true;
#define EXPECT(cond) \
    do { if (!(cond)) { all_of_group = false; printf("  failed at line %d: %s\n", __LINE__, #cond); } } while (0)
static void group(const char* name) {
    printf("%s %s\n", all_of_group ? "ok" : "FAIL", name);
    failures += !all_of_group;
    all_of_group = true;
}

// ---- the six records as the parent commit's kernels read them -----------------------------------------------------------------------
static void records() {
    EXPECT(sizeof(DeletionMeta) == 16 && offsetof(DeletionMeta, t) == 0 && offsetof(DeletionMeta, q) == 4 &&
           offsetof(DeletionMeta, take) == 8 && offsetof(DeletionMeta, s) == 12);
    group("record_DeletionMeta");
    EXPECT(sizeof(LsMeta) == 8 && offsetof(LsMeta, n_inactive) == 0 && offsetof(LsMeta, index_del) == 4);
    group("record_LsMeta");
    EXPECT(sizeof(LsOut) == 40 && offsetof(LsOut, alpha_upp) == 0 && offsetof(LsOut, sums) == 8 && offsetof(LsOut, index_alpha_upp) == 32);
    group("record_LsOut");
    EXPECT(sizeof(PenaltyMeta) == 40 && offsetof(PenaltyMeta, sums) == 0 && offsetof(PenaltyMeta, t) == 24 &&
           offsetof(PenaltyMeta, dimA) == 28 && offsetof(PenaltyMeta, take) == 32 && offsetof(PenaltyMeta, pad) == 36);
    group("record_PenaltyMeta");
    EXPECT(sizeof(PenaltyOut) == 32 && offsetof(PenaltyOut, scalars) == 0 && offsetof(PenaltyOut, branch) == 24 &&
           offsetof(PenaltyOut, pad) == 28);
    group("record_PenaltyOut");
    EXPECT(sizeof(MeritMeta) == 16 && offsetof(MeritMeta, t) == 0 && offsetof(MeritMeta, n_inactive) == 4 &&
           offsetof(MeritMeta, take) == 8 && offsetof(MeritMeta, pad) == 12);
    group("record_MeritMeta");
    EXPECT(LS_SUM_ROWS == 1024 && LS_MAX_NBLK == 64 && BATCH_MAX_T == 1024);
    group("record_constants");
}

// ---- the checks ---------------------------------------------------------------------------------------------------------------------
static void shape_checks() {
    std::string e;
    EXPECT(check_batch(e, 1) == 0 && check_batch(e, 0x7fffffff) == 0 && e.empty());
    EXPECT(check_batch(e, 0) == -2 && e == "batch must be in 1..2^31-1" && check_batch(e, 0x80000000LL) == -2);
    EXPECT(check_l(e, 0) == 0 && check_l(e, 1LL << 27) == 0 && check_l(e, -1) == -3 && e == "l must be in 0..2^27");
    EXPECT(check_l(e, (1LL << 27) + 1) == -3);
    EXPECT(check_t_max(e, 0) == 0 && check_t_max(e, 1024) == 0 && check_t_max(e, 1025) == -3 && check_t_max(e, -1) == -3 &&
           e == "t_max must be in 0..1024 in this build");
    EXPECT(check_shape(e, 4, 12, 12) == 0 && check_shape(e, 4, 11, 12) == -3 && e == "t_max > l");
    EXPECT(check_shape(e, 0, -1, -1) == -2 && check_shape(e, 1, -1, -1) == -3 && e == "l must be in 0..2^27");     // batch, l, t_max
    EXPECT(check_shape(e, 1, 2000, 1025) == -3 && e == "t_max must be in 0..1024 in this build");
    group("shape_checks");
}

static void count_check() {
    for (int64_t batch : {1, 5}) {
        const int64_t lo = 1, hi = 7;
        const Range r{lo, hi, "1..seven"};
        for (int64_t k = 0; k < batch; ++k) {
            std::string e;
            std::unique_ptr<int64_t[]> v(new int64_t[(size_t)batch]);      // exactly batch entries
            for (int64_t i = 0; i < batch; ++i) v[i] = lo;
            v[k] = lo;
            EXPECT(check_count(e, -5, "t", k, v[k], r) == 0 && e.empty());
            v[k] = hi;
            EXPECT(check_count(e, -5, "t", k, v[k], r) == 0 && e.empty());
            v[k] = lo - 1;
            EXPECT(check_count(e, -5, "t", k, v[k], r) == -5);
            EXPECT(e == "t[" + std::to_string(k) + "] outside 1..seven");
            v[k] = hi + 1;
            e.clear();
            EXPECT(check_count(e, -7, "dimA", k, v[k], r) == -7);
            EXPECT(e == "dimA[" + std::to_string(k) + "] outside 1..seven");
        }
    }
    group("count_check");
}

// list: rows of `stride` entries of which row k is allocated up to its LAST USED entry only when it is the last row, and holds
// INT64_MIN behind cnt[k] otherwise
static void list_check() {
    const int64_t l = 9;
    {
        const int64_t batch = 5, stride = 4, cnt[5] = {0, 4, 2, 4, 1};     // cnt == 0, cnt == stride, and a short last row
        std::vector<int64_t> list((size_t)((batch - 1) * stride + cnt[batch - 1]), INT64_MIN);
        for (int64_t k = 0; k < batch; ++k)
            for (int64_t i = 0; i < cnt[k]; ++i) list[(size_t)(k * stride + i)] = 1 + (k + i) % l;
        std::string e;
        for (int64_t k = 0; k < batch; ++k)
            for (int64_t lo : {0, 1}) EXPECT(check_list(e, -6, "active", k, list.data() + k * stride, cnt[k], {lo, l, "x"}) == 0 && e.empty());
        group("list_check_reads_only_the_used_entries");
        list[1 * stride + 3] = l;      // the upper bound itself is legal
        EXPECT(check_list(e, -6, "active", 1, list.data() + 1 * stride, cnt[1], {1, l, "1..l"}) == 0 && e.empty());
        group("list_check_accepts_hi");
        list[3 * stride + 2] = l + 1;
        EXPECT(check_list(e, -6, "active", 3, list.data() + 3 * stride, cnt[3], {1, l, "1..l"}) == -6);
        EXPECT(e == "active[3][2] outside 1..l");
        list[3 * stride + 2] = -1;
        EXPECT(check_list(e, -9, "inactive", 3, list.data() + 3 * stride, cnt[3], {0, l, "0..l"}) == -9);
        EXPECT(e == "inactive[3][2] outside 0..l");
        group("list_check_names_k_and_i");
        list[2 * stride + 1] = 0;
        e.clear();
        EXPECT(check_list(e, -6, "inactive", 2, list.data() + 2 * stride, cnt[2], {0, l, "0..l"}) == 0 && e.empty());
        EXPECT(check_list(e, -6, "inactive", 2, list.data() + 2 * stride, cnt[2], {1, l, "1..l"}) == -6);
        EXPECT(e == "inactive[2][1] outside 1..l");
        group("list_check_lo_is_an_argument");
    }
    {
        const int64_t batch = 3, stride = 0, cnt[3] = {0, 0, 0};
        const int64_t* none = nullptr;
        std::string e;
        for (int64_t k = 0; k < batch; ++k) EXPECT(check_list(e, -6, "active", k, none + k * stride, cnt[k], {1, 0, "1..l"}) == 0);
        group("list_check_null_list_of_stride_0");
    }
}

static void pack() {
    const int64_t batch = 4, stride = 3, cnt[4] = {3, 0, 2, 1};
    std::vector<int64_t> src((size_t)((batch - 1) * stride + cnt[batch - 1]), INT64_MIN);     // the last row ends with its used part
    for (int64_t k = 0; k < batch; ++k)
        for (int64_t i = 0; i < cnt[k]; ++i) src[(size_t)(k * stride + i)] = 10 * (k + 1) + i;
    std::vector<int> dst((size_t)(batch * stride), -7);      // exactly batch * stride ints
    pack_rows(dst.data(), src.data(), cnt, batch, stride);
    bool used = true, padded = true;
    for (int64_t k = 0; k < batch; ++k)
        for (int64_t i = 0; i < stride; ++i) {
            const int got = dst[(size_t)(k * stride + i)];
            if (i < cnt[k]) used = used && got == 10 * (k + 1) + i;
            else padded = padded && got == 0;
        }
    EXPECT(used);
    group("pack_copies_the_used_part");
    EXPECT(padded);
    group("pack_zero_pads");
    std::vector<int> none;
    const int64_t zero[2] = {0, 0};
    pack_rows(none.data(), nullptr, zero, 2, 0);      // stride 0: nothing read, nothing written
    group("pack_stride_0");
}

static void take_and_blocks() {
    const int64_t take[3] = {0, 1, -5};
    EXPECT(take_flag(nullptr, 2) == 1 && take_flag(take, 0) == 0 && take_flag(take, 1) == 1 && take_flag(take, 2) == 1);
    group("take_flag");
    EXPECT(sum_blocks(0) == 0 && sum_blocks(1) == 1 && sum_blocks(1024) == 1 && sum_blocks(1025) == 2 && sum_blocks(64 * 1024 + 1) == 64);
    EXPECT(sum_blocks(63 * 1024 + 1) == 64 && sum_blocks(0x7fffffff) == 64);
    group("sum_blocks");
    const int64_t lim = 0x7fffffff;
    EXPECT(grid_fits(lim, 0) && grid_fits(lim, 1) && !grid_fits(lim + 1, 0) && !grid_fits(lim + 1, 1));
    EXPECT(grid_fits(lim / 64, 64) && !grid_fits(lim / 64 + 1, 64) && grid_fits(1, lim) && !grid_fits(2, lim / 2 + 1));
    group("grid_fits");
}

// ---- the layouts --------------------------------------------------------------------------------------------------------------------
struct Placed {
    std::vector<Carver::Entry> tr;
    std::unique_ptr<char[]> buf;
    size_t bytes = 0;
    const Carver::Entry* find(const char* name) const {
        for (const Carver::Entry& e : tr)
            if (!strcmp(e.name, name)) return &e;
        return nullptr;
    }
};

// as the library runs it: measured, then placed in a buffer of exactly that size, which is written through every array
template <class Layout, class... Shape>
static void place_checked(Layout& L, Placed& P, const Shape&... s) {
    P.bytes = layout_bytes<Layout>(s...);
    P.buf.reset(new char[P.bytes]);
    Carver c;
    c.base = P.buf.get();
    c.trace = &P.tr;
    L.carve(c, s...);
    EXPECT(c.bytes() == P.bytes);
    size_t end = 0;
    for (const Carver::Entry& e : P.tr) {
        EXPECT(e.offset >= end && e.offset % e.align == 0);      // in order, disjoint, aligned as requested
        end = e.offset + e.bytes;
        memset(P.buf.get() + e.offset, 0x5a, e.bytes);
    }
    EXPECT(end <= P.bytes);
}

// the arrays of one copy: equal offsets from the first on both sides, and the byte count from the first one's start to the last
// one's end
static void copy_checked(const Placed& D, const Placed& H, std::initializer_list<const char*> names, size_t d_bytes, size_t h_bytes) {
    const Carver::Entry *d0 = D.find(*names.begin()), *h0 = H.find(*names.begin()), *d1 = nullptr, *h1 = nullptr;
    EXPECT(d0 && h0);
    if (!d0 || !h0) return;
    for (const char* n : names) {
        d1 = D.find(n);
        h1 = H.find(n);
        EXPECT(d1 && h1);
        if (!d1 || !h1) return;
        EXPECT(d1->offset - d0->offset == h1->offset - h0->offset && d1->bytes == h1->bytes);
    }
    EXPECT(d_bytes == d1->offset + d1->bytes - d0->offset);
    EXPECT(h_bytes == h1->offset + h1->bytes - h0->offset);
    EXPECT(h0->offset + h_bytes <= H.bytes && d0->offset + d_bytes <= D.bytes);
}

static void layouts() {
    const int64_t shapes[][4] = {{1, 0, 0, 0}, {3, 2, 5, 1}, {4, 64, 64, 0}, {5, 65, 65, 64}};      // batch, t_max, l, nblk
    for (auto& s : shapes) {
        const int64_t batch = s[0], t_max = s[1], l = s[2], nblk = s[3], none = 0;
        {
            DeletionScratch Dl, Hl;
            Placed D, H;
            place_checked(Dl, D, batch, none, none);
            place_checked(Hl, H, batch, none, none);
            copy_checked(D, H, {"meta", "list"}, Dl.up_bytes, Hl.up_bytes);
            copy_checked(D, H, {"out"}, Dl.down_bytes, Hl.down_bytes);
            EXPECT(Hl.up_bytes == (size_t)batch * sizeof(DeletionMeta) && Hl.down_bytes == (size_t)batch * sizeof(int));
            EXPECT((char*)Dl.meta == D.buf.get() && (char*)Dl.out == D.buf.get() + D.find("out")->offset);
        }
        group("layout_deletion");
        {
            LinesearchScratch Dl, Hl;
            Placed D, H;
            place_checked(Dl, D, batch, l, 3 * nblk);
            place_checked(Hl, H, batch, l, none);
            copy_checked(D, H, {"meta", "list"}, Dl.up_bytes, Hl.up_bytes);
            copy_checked(D, H, {"out"}, Dl.down_bytes, Hl.down_bytes);
            EXPECT(H.find("part")->bytes == 0 && D.find("part")->bytes == (size_t)(batch * 3 * nblk) * sizeof(double));
            EXPECT(Hl.up_bytes == (size_t)batch * (sizeof(LsMeta) + (size_t)l * sizeof(int)) && Hl.down_bytes == (size_t)batch * sizeof(LsOut));
        }
        group("layout_linesearch");
        {
            PenaltyScratch Dl, Hl;
            Placed D, H;
            place_checked(Dl, D, batch, t_max, none);
            place_checked(Hl, H, batch, t_max, none);
            copy_checked(D, H, {"meta", "list"}, Dl.up_bytes, Hl.up_bytes);
            copy_checked(D, H, {"out"}, Dl.down_bytes, Hl.down_bytes);
            EXPECT(Hl.up_bytes == (size_t)batch * (sizeof(PenaltyMeta) + (size_t)t_max * sizeof(int)) &&
                   Hl.down_bytes == (size_t)batch * sizeof(PenaltyOut));
        }
        group("layout_penalty");
        {
            MeritScratch Dl, Hl;
            Placed D, H;
            place_checked(Dl, D, batch, t_max, l, false, nblk);
            place_checked(Hl, H, batch, t_max, l, false, none);
            copy_checked(D, H, {"meta", "act", "inact"}, Dl.up_bytes, Hl.up_bytes);
            copy_checked(D, H, {"psi"}, Dl.down_bytes, Hl.down_bytes);
            EXPECT(H.find("mpart")->bytes == 0 && D.find("mpart")->bytes == (size_t)(batch * nblk) * sizeof(double));
            EXPECT(!H.find("alpha") && !H.find("sums") && !H.find("part") && Hl.psi_bytes == Hl.down_bytes);
            EXPECT(Hl.up_bytes == (size_t)batch * (sizeof(MeritMeta) + (size_t)(t_max + l) * sizeof(int)) &&
                   Hl.down_bytes == (size_t)batch * sizeof(double));
        }
        group("layout_merit");
        {
            MeritScratch Dl, Hl;
            Placed D, H;
            place_checked(Dl, D, batch, t_max, l, true, nblk);
            place_checked(Hl, H, batch, t_max, l, true, none);
            copy_checked(D, H, {"meta", "act", "inact", "alpha"}, Dl.up_bytes, Hl.up_bytes);
            copy_checked(D, H, {"sums", "psi"}, Dl.down_bytes, Hl.down_bytes);
            copy_checked(D, H, {"sums"}, Dl.down_bytes - Dl.psi_bytes, Hl.down_bytes - Hl.psi_bytes);      // a fit without psi_new
            EXPECT(H.find("part")->bytes == 0 && H.find("mpart")->bytes == 0);
            EXPECT(D.find("part")->bytes == (size_t)(batch * nblk * 6) * sizeof(double) && D.find("mpart")->bytes == (size_t)(batch * nblk) * sizeof(double));
            EXPECT(Hl.down_bytes == (size_t)batch * 7 * sizeof(double) && Hl.psi_bytes == (size_t)batch * sizeof(double));
        }
        group("layout_fit");
        {      // the two calls lay the same buffer out: the prefix the merit kernels read is one definition
            MeritScratch M, F;
            Placed PM, PF;
            place_checked(M, PM, batch, t_max, l, false, nblk);
            place_checked(F, PF, batch, t_max, l, true, nblk);
            for (const char* n : {"meta", "act", "inact"}) EXPECT(PM.find(n)->offset == PF.find(n)->offset && PM.find(n)->bytes == PF.find(n)->bytes);
        }
        group("layout_merit_prefix_is_the_fit_prefix");
    }
}

// ---- the working-set lists [active | inactive] of the addition, termination and direction calls -------------------------------------
// source rows of stride l of which row k holds cnt[k] entries 10 (k + 1) + i and INT64_MIN behind them; the last row ends with its
// used part
static std::vector<int64_t> ragged_source(int64_t batch, int64_t l, const std::vector<int64_t>& cnt) {
    std::vector<int64_t> src((size_t)((batch - 1) * l + cnt[(size_t)batch - 1]), INT64_MIN);
    for (int64_t k = 0; k < batch; ++k)
        for (int64_t i = 0; i < cnt[(size_t)k]; ++i) src[(size_t)(k * l + i)] = 10 * (k + 1) + i;
    return src;
}

static void working_sets() {
    {
        int one[1] = {0};
        const WorkingSets<int> w(one, 1, 1), e(one, 1, 0);      // batch = 1; and l = 0, where both halves are empty and coincide
        EXPECT(w.act == one && w.inact == one + 1 && e.act == one && e.inact == one);
        const int64_t big[1] = {0};
        const WorkingSets<const int64_t> c(big, 7, 0);
        EXPECT(c.act == big && c.inact == big);
        std::vector<int> list(2 * 5 * 3);
        const WorkingSets<int> g(list.data(), 5, 3);
        EXPECT(g.act == list.data() && g.inact == list.data() + 15 && g.inact + 15 == list.data() + list.size());
    }
    group("working_sets_halves");
    {
        // t = l (no inactive entry), a problem that is not taken, t = 0 (no active entry), one in between; the sources of the
        // problem that is not taken hold legal-looking entries, which must not arrive
        const int64_t batch = 4, l = 3, t[4] = {3, -1, 0, 2};
        std::vector<int64_t> n_act, n_ina;
        for (int64_t k = 0; k < batch; ++k) { n_act.push_back(t[k] < 0 ? l : t[k]); n_ina.push_back(t[k] < 0 ? l : l - t[k]); }
        std::vector<int64_t> act = ragged_source(batch, l, n_act), ina = ragged_source(batch, l, n_ina);
        std::vector<int> list((size_t)(2 * batch * l), -7);      // exactly both halves
        for (int64_t k = 0; k < batch; ++k) pack_working_sets(list.data(), batch, l, k, act.data(), ina.data(), t[k]);
        const WorkingSets<int> w(list.data(), batch, l);
        bool used = true, padded = true, untaken = true;
        for (int64_t k = 0; k < batch; ++k)
            for (int64_t i = 0; i < l; ++i) {
                const int a = w.act[k * l + i], b = w.inact[k * l + i];
                if (t[k] < 0) { untaken = untaken && a == 0 && b == 0; continue; }
                if (i < t[k]) used = used && a == 10 * (k + 1) + i; else padded = padded && a == 0;
                if (i < l - t[k]) used = used && b == 10 * (k + 1) + i; else padded = padded && b == 0;
            }
        EXPECT(used && padded);
        group("pack_working_sets_t_0_and_t_l");
        EXPECT(untaken);
        group("pack_working_sets_not_taken_rows_are_zero");
    }
    {
        // nothing behind a used count is read: the problem that is not taken comes last and its source rows do not exist
        const int64_t batch = 2, l = 4, t[2] = {1, -1};
        std::vector<int64_t> act = ragged_source(batch, l, {1, 0}), ina = ragged_source(batch, l, {3, 0});
        EXPECT(act.size() == 4 && ina.size() == 4);
        std::vector<int> list((size_t)(2 * batch * l), -7);
        for (int64_t k = 0; k < batch; ++k) pack_working_sets(list.data(), batch, l, k, act.data(), ina.data(), t[k]);
        const int want[16] = {10, 0, 0, 0, 0, 0, 0, 0, 10, 11, 12, 0, 0, 0, 0, 0};
        EXPECT(!memcmp(list.data(), want, sizeof want));
        group("pack_working_sets_reads_only_the_used_entries");
    }
    {
        std::vector<int> none;
        for (int64_t k = 0; k < 3; ++k) pack_working_sets(none.data(), 3, 0, k, nullptr, nullptr, k == 1 ? -1 : 0);      // l = 0
        group("pack_working_sets_l_0");
    }
    {
        // the closing pair of the three per-problem loops: code -7, entries 0..l, active before inactive, the used entries only
        const int64_t batch = 2, l = 3;
        std::vector<int64_t> act = ragged_source(batch, l, {2, 1}), ina = ragged_source(batch, l, {1, 2});
        for (auto* v : {&act, &ina})
            for (int64_t& x : *v) if (x != INT64_MIN) x = x % (l + 1);
        std::string e;
        EXPECT(check_working_set(e, 0, act.data(), ina.data(), l, 2) == 0 && check_working_set(e, 1, act.data(), ina.data(), l, 1) == 0 && e.empty());
        ina[(size_t)(1 * l + 1)] = l + 1;
        EXPECT(check_working_set(e, 1, act.data(), ina.data(), l, 1) == -7 && e == "inactive[1][1] outside 0..l");
        act[(size_t)(1 * l)] = -1;
        EXPECT(check_working_set(e, 1, act.data(), ina.data(), l, 1) == -7 && e == "active[1][0] outside 0..l");
        e.clear();
        EXPECT(check_working_set(e, 0, act.data(), ina.data(), l, 2) == 0 && e.empty());
        EXPECT(check_working_set(e, 0, nullptr, nullptr, 0, 0) == 0 && e.empty());
        group("check_working_set");
    }
}

// the preamble of check_addition / check_termination / check_direction: batch, m, n, l <= 1024, t_max, t_max > l in this order, with
// the messages and codes that tests/addition_walk_check.cpp, termination_check.cpp and direction_check.cpp pin for the callers; each
// caller gives exactly the preamble's answer (nothing else of its arguments is looked at before)
static void working_set_shape() {
    struct Case { int64_t batch, m, n, l, t_max; int rc; const char* msg; };
    const Case cases[] = {
        {2, 9, 4, 5, 3, 0, ""},
        {1, 0, 1, 0, 0, 0, ""},
        {1, 0x7fffffff, 0x3fffffff, 1024, 1024, 0, ""},
        {0, 9, 4, 5, 3, -2, "batch must be in 1..2^31-1"},
        {0x80000000LL, 9, 4, 5, 3, -2, "batch must be in 1..2^31-1"},
        {2, -1, 4, 5, 3, -3, "m must be in 0..2^31-1"},
        {2, 0x80000000LL, 4, 5, 3, -3, "m must be in 0..2^31-1"},
        {2, 9, 0, 5, 3, -3, "n must be at least 1"},
        {2, 9, 0x40000000, 5, 3, -3, "n must be at least 1"},
        {2, 9, 4, -1, 0, -3, "l must be in 0..1024 in this build"},
        {2, 9, 4, 1025, 3, -3, "l must be in 0..1024 in this build"},
        {2, 9, 4, 5, -1, -3, "t_max must be in 0..1024 in this build"},
        {2, 9, 4, 5, 6, -3, "t_max > l"},
        // two faults at once: the earlier one of the order wins
        {0, -1, 0, 1025, 1025, -2, "batch must be in 1..2^31-1"},
        {2, -1, 0, 1025, 1025, -3, "m must be in 0..2^31-1"},
        {2, 9, 0, 1025, 1025, -3, "n must be at least 1"},
        {2, 9, 4, 1025, 1026, -3, "l must be in 0..1024 in this build"},
        {2, 9, 4, 1024, 1025, -3, "t_max must be in 0..1024 in this build"},
    };
    bool pre = true, add = true, term = true, dir = true;
    for (const Case& c : cases) {
        std::string e;
        pre = pre && check_working_set_shape(e, c.batch, c.m, c.n, c.l, c.t_max) == c.rc && e == c.msg;
        if (c.rc == 0) continue;      // a good shape goes on to the callers' own arguments: their own groups
        e.clear();
        term = term && check_termination(e, {c.batch, c.m, c.n, c.l, c.t_max, 0, 0, 0, 0}, nullptr, nullptr, nullptr, nullptr, false,
                                         false, false, false, false) == c.rc && e == c.msg;
        e.clear();
        dir = dir && check_direction(e, {c.batch, c.m, c.n, c.l, c.t_max}, nullptr, nullptr, nullptr, nullptr, false, false, false,
                                     false) == c.rc && e == c.msg;
        if (c.m < 0 || c.m > 0x7fffffff) continue;      // the addition call has no m
        e.clear();
        add = add && check_addition(e, {c.batch, c.n, c.l, c.t_max, 0, 0, 0, 0}, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                    false, false, false) == c.rc && e == c.msg;
    }
    EXPECT(pre);
    group("working_set_shape");
    EXPECT(add);
    group("working_set_shape_of_check_addition");
    EXPECT(term);
    group("working_set_shape_of_check_termination");
    EXPECT(dir);
    group("working_set_shape_of_check_direction");
    std::string e;
    EXPECT(check_m(e, 0) == 0 && check_n(e, 1) == 0 && check_t_max_in_l(e, 0, 0) == 0 && check_t_max_in_l(e, 1024, 1024) == 0 && e.empty());
    EXPECT(check_t_max_in_l(e, 1025, 1024) == -3 && e == "t_max must be in 0..1024 in this build");
    EXPECT(check_t_max_in_l(e, 3, 2) == -3 && e == "t_max > l");
    group("shape_pieces");
}

int main() {
    records();
    shape_checks();
    count_check();
    list_check();
    pack();
    take_and_blocks();
    layouts();
    working_sets();
    working_set_shape();
    printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
