// Shape plan of a batch (batch, m, n, t) and the layouts of the workspaces whose sizes follow from it.  Host-only (gn_layout.hpp).
#pragma once
#include <algorithm>
#include <vector>

#include "gn_layout.hpp"

namespace gn {

// what the layouts must know of the device side; enlsip_gn.hip asserts that they are the kernels' own values
constexpr int PLAN_PB = 32, PLAN_KBLK = 64, PLAN_QD_CPW = 8;
constexpr long long PLAN_PAIR_MIN_WGS = 8192;      // the pair rule of plan_geometry
constexpr size_t PLAN_STATE_BYTES = 32, PLAN_SBINFO_BYTES = 32, PLAN_QDCAND_BYTES = 16, PLAN_SMALL_BYTES = 256;
struct ProbState;
struct SmallScalars;

inline long long rup(long long x, long long a) { return (x + a - 1) / a * a; }
inline long long pad32(long long x) { return rup(std::max<long long>(x, 1), 32); }   // 256-byte granules of doubles

struct LevelPlan {
    int level;
    int nblocks;      // 32-row blocks entering this level
    int groups;       // workgroups (= blocks of the next level)
    long long S;      // block stride (rows)
    long long tOff;   // first T block index
    int mode = 0;     // row geometry (CaqrArgs::mode): 0 level-0 tiles, 1 plain tree level, 2 first tree level of a pair's second panel
    long long base = 0;   // row of block 0
    int skip = 0;     // level 0: leading 32-row units of every tile that belong to the pair's first panel
};
struct PanelPlan {
    std::vector<LevelPlan> levels;
};

struct Plan {
    long long batch = 0, m = 0, n = 0, t = 0;
    int kA = 0;
    int RPL = 8;         // CAQR rows per lane (tile rows = 64 * RPL)
    int F = 16;          // blocks per group
    int ldw = 0, ldr = 0;
    int npan_max = 0;    // panels if n2 = n
    bool pair = false;   // panels (2K, 2K+1) share their tiles and one pass over the far trailing columns (gn_kernels_caqr.hpp, "Panel pairs")
    long long nTblocks = 0;
    std::vector<PanelPlan> panels;
    // per-problem strides (elements)
    long long sFA, sTauA, sJA, sFL, sTauL, sJL, sTA, sP1, sB, sW, sT, sRt, sTauJ, sJJ, sZ, sVec;
    // distributed pivoted QR (gn_kernels_qrcp_dist.hpp)
    long long sM, sVb, sDiag, sVn, sQI, sCand, sAct;
    int qdGmax = 0;
};

// geometry of (batch, m, n, t): tiles, leading dimensions, panel and level lists, the pair rule, the strides
inline Plan plan_geometry(long long batch, long long m, long long n, long long t, int tile_rows, bool update_reflectors,
                          bool pair_enabled, bool pair_forced) {
    Plan P;
    P.batch = batch; P.m = m; P.n = n; P.t = t;
    P.kA = (int)std::min(n, t);
    P.RPL = (m <= 256 ? 256 : tile_rows) / 64;      // a problem of at most 256 rows is one 256-row tile
    P.F = 2 * P.RPL;
    P.ldw = (int)pad32(m);
    // a leading dimension that is a multiple of 4 KB puts the same row range of every column on the
    // same few HBM channels (measured: 4x slower edge tiles at ldw = 4096): skew it by one 256-B block
    if (P.ldw % 512 == 0) P.ldw += 32;
    const long long kpmax = std::min(m, n);
    P.ldr = (int)rup(std::max<long long>(kpmax, 1), 8);
    P.npan_max = (int)((kpmax + PLAN_PB - 1) / PLAN_PB);
    long long running = 0;
    P.panels.resize(P.npan_max);
    // panel pairs (gn_kernels_caqr.hpp): from three panels on; the reflector-by-reflector A/B path keeps the plain sweep
    // ... and only where the far update is the bulk of the sweep: the pair costs two extra small launches per two panels
    // (the first panel's level-0 and tree reflectors on the second panel's 32 columns), which a latency-bound sweep does not
    // earn back.  Measured (MI355X): 384 x C2 +1.4 % solves/s and C4's 262144 rows 29.7 -> 27.4 ms with pairs, but a single
    // C2 problem 5.17 -> 5.37 ms, 64 of them 10.35 -> 10.47 ms, a 32768-row C4 shard 16.8 -> 17.2 ms.  Rule: at least ~8192
    // far-update workgroups in the first pair (tiles x 32-column blocks x problems); ENLSIP_GN_PAIR=1 forces pairs.
    const long long far_wgs = batch * ((std::max<long long>(m, 1) + 64 * P.RPL - 1) / (64 * P.RPL)) * ((std::max<long long>(n - P.kA, 1) + 31) / 32);
    P.pair = pair_enabled && !update_reflectors && P.npan_max >= 3 && (far_wgs >= PLAN_PAIR_MIN_WGS || pair_forced);
    const long long mpad = pad32(m);    // NOT ldw: the skew rows are never touched
    for (int k = 0; k < P.npan_max; ++k) {
        const bool second = P.pair && (k & 1);                    // second panel of the pair (k - 1, k): keeps the first one's tiles
        const long long anchor = 32LL * (k - (second ? 1 : 0));   // first row of tile 0
        const int nb0 = (int)((mpad - anchor) / 32);              // 32-row blocks from the anchor to the padded m
        const int ntiles = (nb0 + P.F - 1) / P.F;
        const int last_units = nb0 - (ntiles - 1) * P.F;          // blocks of the last tile
        auto push = [&](int level, int mode, long long base, int skip, int nblocks, int groups, long long S) {
            LevelPlan L;
            L.level = level; L.mode = mode; L.base = base; L.skip = skip;
            L.nblocks = nblocks; L.groups = groups; L.S = S;
            L.tOff = running;
            running += groups;
            P.panels[k].levels.push_back(L);
        };
        // level 0: the tiles (a tile that has no row of the second panel still gets its — zero — T block: the pair update indexes
        // T by tile)
        push(0, 0, anchor, second ? 1 : 0, nb0, ntiles, 32);
        if (ntiles <= 1) continue;
        int level = 1, nb;
        long long S = 32LL * P.F, base = 32LL * k;
        if (!second) nb = ntiles;
        else {
            // first tree level of the second panel: per tile the new R factor (rows 32..63) and, from tile 1 on, the rows 0..31
            // the first panel's tree left behind (dense in these columns): mode 2
            const int nblocks1 = (ntiles - (last_units == 1 ? 1 : 0)) + (ntiles - 1);
            const int groups1 = (nblocks1 + P.F - 1) / P.F;
            push(1, 2, anchor, 0, nblocks1, groups1, S);
            if (groups1 <= 1) continue;
            // group leaders: blocks F q of level 1 = (tile (F / 2) q, rows 32..63)
            nb = groups1;
            S = S * (P.F / 2);
            level = 2;
        }
        while (true) {
            const int groups = (nb + P.F - 1) / P.F;
            push(level, 1, base, 0, nb, groups, S);
            if (groups <= 1) break;
            nb = groups;
            S *= P.F;
            ++level;
        }
    }
    P.nTblocks = std::max<long long>(running, 1);
    const long long nblkA = std::max<long long>((P.kA + PLAN_KBLK - 1) / PLAN_KBLK, 1);
    P.sFA = pad32(n * t); P.sTauA = pad32(P.kA); P.sJA = pad32(t);
    P.sFL = pad32(t * P.kA); P.sTauL = pad32(P.kA); P.sJL = pad32(P.kA);
    P.sTA = pad32(nblkA * PLAN_KBLK * PLAN_KBLK); P.sP1 = pad32(t); P.sB = pad32(t);
    // 32 spare columns per problem: the trailing-update kernel (k_caqr_update*) reads (and discards) whole 32-column blocks
    P.sW = pad32((long long)P.ldw * (n + 1 + 32));
    P.sT = pad32(P.nTblocks * PLAN_PB * PLAN_PB);
    P.sRt = pad32((long long)P.ldr * (n + 1));
    P.sTauJ = pad32(kpmax); P.sJJ = pad32(n); P.sZ = pad32(kpmax);
    P.sVec = pad32((long long)P.ldw * 2);
    // + 33 columns: k_sb_update_blk reads whole 32-column / 32-row blocks past the last valid element
    P.sM = pad32((long long)P.ldr * (n + 1 + 33)); P.sVb = pad32((long long)P.ldr * (std::max<long long>(kpmax, 1) + 33));
    P.sDiag = pad32(kpmax); P.sVn = pad32(n); P.sQI = pad32(n);
    P.sAct = P.sQI + 32;      // the active list has n + 1 entries (the columns and the right-hand side)
    P.qdGmax = (int)((n + 1 + PLAN_QD_CPW - 1) / PLAN_QD_CPW);
    P.sCand = 2 * (long long)P.qdGmax;
    return P;
}

// ---- the main workspace (h->ws): the handle IS this set of pointers.  The order and the alignments are the placement the HBM
// channel tuning was done on (see ldw above): a new array goes at the END.
struct WsLayout {
    double *W = nullptr, *FA = nullptr, *tauA = nullptr, *FL = nullptr, *tauL = nullptr, *TA = nullptr, *p1 = nullptr,
           *bvec = nullptr, *Tbuf = nullptr, *Rt = nullptr, *tauJ = nullptr, *zsave = nullptr, *vec = nullptr, *qdM = nullptr,
           *qdVb = nullptr, *qdDiag = nullptr, *qdVn1 = nullptr, *qdVn2 = nullptr;
    double* sbT = nullptr;               // per problem: T factor of the current QRCP block (32 x 32)
    long long *jpvtA = nullptr, *jpvtL = nullptr, *jpvtJ = nullptr;
    int *qdChosen = nullptr, *qdPos = nullptr, *qdColat = nullptr;
    void* qdCand = nullptr;              // QdCand
    ProbState* state = nullptr;
    SmallScalars* small = nullptr;       // device scalars of the handle
    void* sbInfo = nullptr;              // SbInfo per problem (device)
    int* sbInblk = nullptr;              // per column block id (device)
    int* sbAct = nullptr;                // per problem: columns the current block update touches (device)

    void carve(Carver& c, const Plan& P) {
        const size_t b = (size_t)P.batch;
        c.take(W, "W", b * P.sW, 256);
        c.take(FA, "FA", b * P.sFA, 256); c.take(tauA, "tauA", b * P.sTauA, 256);
        c.take(FL, "FL", b * P.sFL, 256); c.take(tauL, "tauL", b * P.sTauL, 256);
        c.take(TA, "TA", b * P.sTA, 256); c.take(p1, "p1", b * P.sP1, 256); c.take(bvec, "bvec", b * P.sB, 256);
        c.take(Tbuf, "Tbuf", b * P.sT, 256); c.take(Rt, "Rt", b * P.sRt, 256); c.take(tauJ, "tauJ", b * P.sTauJ, 256);
        c.take(zsave, "zsave", b * P.sZ, 256); c.take(vec, "vec", b * P.sVec, 256);
        c.take(qdM, "qdM", b * P.sM, 256); c.take(qdVb, "qdVb", b * P.sVb, 256); c.take(qdDiag, "qdDiag", b * P.sDiag, 256);
        c.take(qdVn1, "qdVn1", b * P.sVn, 256); c.take(qdVn2, "qdVn2", b * P.sVn, 256);
        c.take(sbT, "sbT", b * PLAN_PB * PLAN_PB, 256);
        c.take(jpvtA, "jpvtA", b * P.sJA, 256); c.take(jpvtL, "jpvtL", b * P.sJL, 256); c.take(jpvtJ, "jpvtJ", b * P.sJJ, 256);
        // 32-bit arrays: strides of 128 bytes, packed
        c.take(qdChosen, "qdChosen", b * P.sQI, 128);
        c.take(qdPos, "qdPos", b * 2 * P.sQI, 128);
        c.take(qdColat, "qdColat", b * 2 * P.sQI, 128);
        qdCand = c.raw("qdCand", b * P.sCand * PLAN_QDCAND_BYTES, 16);
        state = (ProbState*)c.raw("state", (size_t)rup((long long)(b * PLAN_STATE_BYTES), 256), 32);
        small = (SmallScalars*)c.raw("small", PLAN_SMALL_BYTES, 32);
        sbInfo = c.raw("sbInfo", (size_t)rup((long long)(b * PLAN_SBINFO_BYTES), 256), 32);
        c.take(sbInblk, "sbInblk", b * P.sQI, 32);
        c.take(sbAct, "sbAct", b * P.sAct);
    }
};

// ---- workspace of the distributed constraint stage (h->cws, run_constraint_dist): every array on a 256-byte boundary
struct CwsLayout {
    long long ldc = 0, sM = 0, sVb = 0, sRt = 0, sL = 0, sVec = 0, sI = 0, sCand = 0;    // strides (elements)
    int G = 0;
    double *M = nullptr, *Vb = nullptr, *Rt = nullptr, *L = nullptr, *diag = nullptr, *vn1 = nullptr, *vn2 = nullptr;
    double *bq = nullptr, *qb = nullptr;     // b_buff, later F_L11.Q' b_buff
    int *chosen = nullptr, *pos = nullptr, *colat = nullptr;
    void* cand = nullptr;                    // QdCand
    ProbState *stA = nullptr, *stL = nullptr;

    void carve(Carver& c, long long batch, long long n, long long t, int kA) {
        const size_t b = (size_t)batch;
        ldc = rup(std::max(n, t), 8);
        sM = pad32(ldc * (t + 2)); sVb = pad32(ldc * (kA + 1)); sRt = pad32(ldc * (t + 2)); sL = pad32(ldc * (kA + 1));
        sVec = pad32(std::max(n, t) + 1); sI = pad32(t + 1);
        G = (int)((t + 1 + PLAN_QD_CPW - 1) / PLAN_QD_CPW);
        sCand = 2LL * G;
        c.take(M, "cM", b * sM, 256); c.take(Vb, "cVb", b * sVb, 256); c.take(Rt, "cRt", b * sRt, 256); c.take(L, "cL", b * sL, 256);
        c.take(diag, "cDiag", b * sVec, 256); c.take(vn1, "cVn1", b * sVec, 256); c.take(vn2, "cVn2", b * sVec, 256);
        c.take(bq, "cBq", b * sVec, 256); c.take(qb, "cQb", b * sVec, 256);
        c.take(chosen, "cChosen", b * sI, 256); c.take(pos, "cPos", b * 2 * sI, 256); c.take(colat, "cColat", b * 2 * sI, 256);
        cand = c.raw("cCand", b * sCand * PLAN_QDCAND_BYTES, 256);
        stA = (ProbState*)c.raw("stA", b * PLAN_STATE_BYTES, 256);
        stL = (ProbState*)c.raw("stL", b * PLAN_STATE_BYTES, 256);
    }
};

// ---- staging of the host-pointer entry points: inputs packed (ld = m / n) in h->in_stage, outputs packed in h->out_stage.
// One description for every entry point, so that a solve that follows a constraint call finds A', cx in their slots.
struct StageIn {
    double *J = nullptr, *rx = nullptr, *At = nullptr, *cx = nullptr;
    void carve(Carver& c, long long batch, long long m, long long n, long long t) {
        const size_t b = (size_t)batch;
        c.take(J, "J", b * m * n); c.take(rx, "rx", b * m); c.take(At, "At", b * n * t); c.take(cx, "cx", b * t);
    }
};
struct StageOut {
    double *p = nullptr, *b = nullptr, *d = nullptr;
    long long *jA = nullptr, *jL = nullptr, *jJ = nullptr;
    void carve(Carver& c, long long batch, long long m, long long n, long long t) {
        const size_t k = (size_t)batch;
        c.take(p, "p", k * n); c.take(b, "b", k * t); c.take(d, "d", k * m);
        c.take(jA, "jpvtA", k * t); c.take(jL, "jpvtL", k * std::min(n, t)); c.take(jJ, "jpvtJ2", k * n);
    }
};

// ---- the stacked problem of the TSQR combine stage in h->scratch
struct TsqrScratch {
    double *Jst = nullptr, *rxs = nullptr, *p2 = nullptr, *d = nullptr, *pout = nullptr;
    void carve(Carver& c, long long G, long long n2, long long n) {
        const size_t ms = (size_t)G * n2;
        c.take(Jst, "Jst", ms * n2); c.take(rxs, "rxs", ms); c.take(p2, "p2", (size_t)n2); c.take(d, "d", ms); c.take(pout, "pout", (size_t)n);
    }
};

// ---- the Newton direction of one problem in h->newton
struct NewtonWs {
    double *G = nullptr, *Q = nullptr, *T1 = nullptr, *E = nullptr, *W22 = nullptr, *Ut = nullptr, *W21 = nullptr, *g = nullptr,
           *d = nullptr, *p2 = nullptr, *pout = nullptr;
    int* flag = nullptr;     // 4 words
    void carve(Carver& c, long long n, long long n2, long long rankA) {
        const size_t nn = (size_t)n * n, n22 = (size_t)n2 * n2;
        c.take(G, "Gam", nn); c.take(Q, "Q", nn); c.take(T1, "T1", nn); c.take(E, "E", nn);
        c.take(W22, "W22", n22); c.take(Ut, "Ut", n22); c.take(W21, "W21", (size_t)n2 * std::max<long long>(rankA, 1));
        c.take(g, "g", (size_t)n2); c.take(d, "d", (size_t)n2); c.take(p2, "p2", (size_t)n2); c.take(pout, "pout", (size_t)n);
        c.take(flag, "flag", 4, 8);
    }
};

}  // namespace gn
