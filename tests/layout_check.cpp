// Prints every array of the host-side workspace layouts (gn_plan.hpp) for the shapes of tests/test_workspace_layout_host.py: one JSON
// line per array {layout, shape, name, offset, bytes, align} and one per layout {layout, shape, measured}.  Each layout runs as the
// library runs it: once without a base (the byte count), once placed in a buffer of exactly that many bytes, which is then written
// from end to end through the placed pointers' byte ranges, so that the sanitizers see any array that leaves the buffer.
#include <cstdio>
#include <cstring>
#include <string>

#include "../enlsip.jl_amd/csrc/gn_layout.hpp"
#include "../enlsip.jl_amd/csrc/gn_plan.hpp"

using namespace gn;

template <class Layout, class... Shape>
static void report(const char* layout, const std::string& shape, const Shape&... s) {
    const size_t measured = layout_bytes<Layout>(s...);
    // a real buffer for the small shapes; the large ones (GBs) are placed on a fake base and never dereferenced
    const bool real = measured <= (64u << 20);
    std::vector<char> buf(real ? measured : 0);
    std::vector<Carver::Entry> tr;
    Layout L;
    Carver c;
    c.base = real ? buf.data() : (char*)(size_t)(1ull << 40);
    c.trace = &tr;
    L.carve(c, s...);
    for (const Carver::Entry& e : tr) {
        if (real) memset(buf.data() + e.offset, 0x5a, e.bytes);
        printf("{\"layout\": \"%s\", \"shape\": \"%s\", \"name\": \"%s\", \"offset\": %zu, \"bytes\": %zu, \"align\": %zu}\n", layout,
               shape.c_str(), e.name, e.offset, e.bytes, e.align);
    }
    printf("{\"layout\": \"%s\", \"shape\": \"%s\", \"measured\": %zu, \"placed_end\": %zu}\n", layout, shape.c_str(), measured, c.bytes());
}

int main() {
    struct S { long long batch, m, n, t; int tile_rows; bool forced; };
    const S shapes[] = {
        {1, 1, 1, 0, 512, false}, {3, 33, 32, 1, 512, false}, {3, 512, 64, 8, 512, false}, {2, 4096, 512, 64, 512, false},
        {2, 1056, 100, 0, 512, true}, {2, 1056, 100, 0, 256, true}, {1, 40000, 1024, 0, 512, true}, {2, 200, 128, 65, 512, false},
        {1, 1024, 1024, 1024, 512, false},
        // the benchmark configurations (C1: the 3 x 3 plumbing problem; C2 .. C5: workload.CONFIGS)
        {1, 3, 3, 0, 512, false}, {384, 4096, 512, 64, 512, false}, {1024, 512, 64, 8, 512, false}, {1, 262144, 1024, 0, 512, false},
        {8192, 256, 32, 4, 512, false}};
    for (const S& s : shapes) {
        char key[96];
        snprintf(key, sizeof key, "%lld,%lld,%lld,%lld,%d,%d", s.batch, s.m, s.n, s.t, s.tile_rows, (int)s.forced);
        const Plan P = plan_geometry(s.batch, s.m, s.n, s.t, s.tile_rows, false, true, s.forced);
        printf("{\"layout\": \"plan\", \"shape\": \"%s\", \"pair\": %s}\n", key, P.pair ? "true" : "false");
        report<WsLayout>("ws", key, P);
        report<CwsLayout>("cws", key, s.batch, s.n, s.t, P.kA);
        report<StageIn>("stage_in", key, s.batch, s.m, s.n, s.t);
        report<StageOut>("stage_out", key, s.batch, s.m, s.n, s.t);
    }
    const long long tsqr[][2] = {{1, 1}, {3, 7}, {8, 1024}};
    for (auto& g : tsqr) report<TsqrScratch>("tsqr", std::to_string(g[0]) + "," + std::to_string(g[1]), g[0], g[1], (long long)1024);
    const long long newton[][3] = {{1, 1, 0}, {5, 3, 2}, {64, 64, 0}};
    for (auto& g : newton)
        report<NewtonWs>("newton", std::to_string(g[0]) + "," + std::to_string(g[1]) + "," + std::to_string(g[2]), g[0], g[1], g[2]);
    return 0;
}
