// A host model of the capturable layer launch's gate protocol (compactfusion_amd/csrc/cfx_capture_gate.h: the ONLY project header this
// program includes - the kernels of csrc/cfx_capture.hip and this model read the same three functions).  Stand-alone: its own main, built by
// tests/test_captured_layer_host.py with the host compiler and -fsanitize=address,undefined, run as its own process; exit 0 = every
// assertion held.
//
// One slot, launches in stream order (launch r + 1 starts when every workgroup of launch r has left), and inside a launch a seeded random
// interleaving of: the n_st arrivals of group S, the entry tickets of the items x n_dw workgroups of group D - drawn before, among and after
// the arrivals -, and the polls of the D workgroups, some of which give up (they have drawn their ticket and leave without passing).
// Asserted: every workgroup derives its launch's number; the "open" words are written exactly once per launch, with r + 1; a workgroup
// passes only the gate of its own launch - after all n_st arrivals of that launch - whether it is its XCD's relay (claim word), polls the
// relay's local word or falls back on the fabric word.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "cfx_capture_gate.h"

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "capture_gate_model: %s:%d: %s (n_st %u n_dw %u items %d launch %llu seed %u)\n", \
                                               __FILE__, __LINE__, #c, g_n_st, g_n_dw, g_items, (unsigned long long)g_launch, g_seed); std::exit(1); } } while (0)
static unsigned g_n_st, g_n_dw, g_seed;
static int g_items;
static cfx_cap_u64 g_launch;

struct Slot {                                  // the words of a slot the protocol touches (all zero: before launch 0)
    cfx_cap_u64 arrivals;
    unsigned open[8], local[8], claim[8];
    cfx_cap_u64 ticket[CFX_CAP_MAX_ITEMS];
};

struct DWg { int item; int xcd; bool drew, relay, done, gives_up; unsigned expect; int polls; };

static long run(unsigned n_st, unsigned n_dw, int items, unsigned seed, int launches) {
    g_n_st = n_st; g_n_dw = n_dw; g_items = items; g_seed = seed;
    std::mt19937 rng(seed);
    Slot s;
    std::memset(&s, 0, sizeof(s));
    long passed = 0;
    for (cfx_cap_u64 L = 0; L < (cfx_cap_u64)launches; ++L) {
        g_launch = L;
        unsigned arrived = 0;
        int open_writes = 0;
        std::vector<DWg> d((size_t)items * n_dw);
        for (size_t i = 0; i < d.size(); ++i) {
            d[i] = DWg{(int)(i / n_dw), (int)(rng() % 8), false, false, false, rng() % 7 == 0, 0u, 0};
        }
        // how eager group D is this launch: its tickets mostly before, among or after the arrivals
        const unsigned bias = rng() % 3;           // 0: D first, 1: mixed, 2: S first
        size_t left = d.size();
        while (arrived < n_st || left) {
            const bool pick_s = arrived < n_st && (!left || (bias == 0 ? rng() % 8 == 0 : bias == 1 ? rng() % 2 == 0 : rng() % 8 != 0));
            if (pick_s) {
                // a workgroup of group S: ONE fetch-add; its number, and whether it is the launch's last arriver
                const cfx_cap_u64 old = s.arrivals++;
                const cfx_cap_u64 r = cfx_cap_launch(old, n_st);
                CHECK(r == L);
                CHECK(cfx_cap_last(old, n_st) == ((old + 1) % n_st == 0));
                ++arrived;
                if (cfx_cap_last(old, n_st)) {
                    CHECK(arrived == n_st);
                    for (int x = 0; x < 8; ++x) { CHECK(s.open[x] == (unsigned)L); s.open[x] = cfx_cap_expect(r); }
                    ++open_writes;
                } else CHECK(arrived < n_st);
                continue;
            }
            // a step of a random unfinished workgroup of group D
            size_t k = rng() % d.size();
            while (d[k].done) k = (k + 1) % d.size();
            DWg& w = d[k];
            if (!w.drew) {
                const cfx_cap_u64 t = s.ticket[w.item]++;
                const cfx_cap_u64 r = cfx_cap_launch(t, n_dw);
                CHECK(r == L);
                w.expect = cfx_cap_expect(r);
                CHECK(w.expect == (unsigned)(L + 1));
                w.drew = true;
                // gate_wait's relay claim: the first of its XCD to exchange the launch's value in
                const unsigned was = s.claim[w.xcd];
                s.claim[w.xcd] = w.expect;
                w.relay = was != w.expect;
                continue;
            }
            ++w.polls;
            if (w.gives_up && w.polls > 3) { w.done = true; --left; continue; }      // a wait that timed out: ticket drawn, nothing passed
            bool pass;
            if (w.relay) {
                pass = s.open[w.xcd] == w.expect;
                if (pass) s.local[w.xcd] = w.expect;
            } else {
                pass = s.local[w.xcd] == w.expect || (w.polls % 16 == 0 && s.open[w.xcd] == w.expect);
            }
            if (pass) {
                CHECK(arrived == n_st);            // only this launch's gate, and only once it is open
                CHECK(open_writes == 1);
                w.done = true; --left; ++passed;
            } else if (arrived == n_st && w.polls > 64 && !w.relay) {
                // (a relay that gave up never writes the local word: the fabric word is the fallback)
                pass = s.open[w.xcd] == w.expect;
                CHECK(pass);
                w.done = true; --left; ++passed;
            }
        }
        CHECK(open_writes == 1);
        CHECK(s.arrivals == (L + 1) * n_st);
        for (int i = 0; i < items; ++i) CHECK(s.ticket[i] == (L + 1) * n_dw);
        for (int x = 0; x < 8; ++x) CHECK(s.open[x] == (unsigned)(L + 1));
    }
    return passed;
}

int main() {
    // the arithmetic at the edges: a single workgroup, the value that wraps at 32 bits, counters far beyond 32 bits
    g_n_st = g_n_dw = 1; g_items = 0; g_seed = 0; g_launch = 0;
    CHECK(cfx_cap_launch(0, 1) == 0 && cfx_cap_last(0, 1) && cfx_cap_expect(0) == 1u);
    CHECK(cfx_cap_launch(9, 10) == 0 && cfx_cap_last(9, 10) && !cfx_cap_last(8, 10) && cfx_cap_launch(10, 10) == 1 && !cfx_cap_last(10, 10));
    CHECK(cfx_cap_expect(0xFFFFFFFFull) == 0u && cfx_cap_expect(0xFFFFFFFEull) == 0xFFFFFFFFu && cfx_cap_expect(0x100000000ull) == 1u);
    CHECK(cfx_cap_launch(0x100000000ull * 10 + 3, 10) == 0x100000000ull && cfx_cap_last(0x100000000ull * 10 + 9, 10));
    CHECK(CFX_CAP_TICKET_OFF + CFX_CAP_MAX_ITEMS * CFX_CAP_LINE == CFX_CAP_SLOT_WORDS && CFX_CAP_SLOT_WORDS % CFX_CAP_LINE == 0);
    const unsigned NST[] = {1, 2, 10}, NDW[] = {1, 3};
    long passed = 0;
    unsigned seed = 20260;
    for (unsigned n_st : NST)
        for (unsigned n_dw : NDW)
            for (int items = 1; items <= 4; ++items)
                for (int rep = 0; rep < 3; ++rep) passed += run(n_st, n_dw, items, ++seed, 200);
    std::printf("capture_gate_model: ok, %ld gates passed\n", passed);
    return 0;
}
