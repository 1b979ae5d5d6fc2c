// The arithmetic of the CAPTURABLE layer launch of the block-local codecs (cfx_capture.hip; include/cfx.h "Stream capture",
// cfx_set_captured_layer): the launch number a workgroup derives ON THE DEVICE from counters that only ever grow, so that a replayed hipGraph
// node waits for the numbers of ITS replay and nothing is advanced or reset by anybody.  Plain C++ as well as HIP: the host (the pool's
// bookkeeping, tests/capture_gate_model.cpp) and the kernels read the same three functions.
//
// A capturable launch owns a private gate SLOT (CFX_CAP_SLOT_WORDS u32 words, all zero = before launch 0) that no other launch - eager or
// captured - ever uses; every launch of the slot is the same graph node, so it has the same geometry: n_st workgroups in group S, n_dw
// workgroups per reconstruction item in group D.
//   group S   arrives with ONE 64-bit fetch-add of 1 on the slot's arrival counter.  From the returned `old`: the launch's number is
//             cfx_cap_launch(old, n_st); the arriver with cfx_cap_last(old, n_st) is the launch's last and writes cfx_cap_expect(r) to the
//             eight per-XCD "open" words.
//   group D   draws an entry ticket: ONE 64-bit fetch-add of 1 on the counter of its ITEM (a line of its own: not the arrival counter's, and
//             no two items share one).  The launch's number is cfx_cap_launch(ticket, n_dw); it waits for cfx_cap_expect(r).
// Launches of one slot are stream-ordered, so the n_st arrivals and the n_dw tickets per item of launch r are all drawn before any of
// launch r + 1: the counters' values [r * n, (r + 1) * n) belong to launch r.  A workgroup whose wait gives up has drawn its ticket before,
// and group S never waits before it arrives: a time-out leaves the slot consistent.
// Wrap: the counters are 64-bit and count ONE per workgroup and launch - at 10^9 arrivals a second they last 584 years.  The value waited
// for is 32 bits of r + 1: every wait compares for EQUALITY with a word that holds the previous launch's value (or, the peer-to-peer
// exchange, a signed 32-bit difference), and r and r + 1 differ modulo 2^32, so its wrap after 2^32 launches of a slot changes nothing.
#ifndef CFX_CAPTURE_GATE_H
#define CFX_CAPTURE_GATE_H

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CFX_CAP_HD __host__ __device__
#else
#define CFX_CAP_HD
#endif

typedef unsigned long long cfx_cap_u64;

// Layout of a slot in u32 words (64-byte lines of 16): the gate block of cfx_device.h's gate_wait (the arrival counter's line - here a u64 -,
// then per XCD an "open", a local and a relay claim word, a line each), a second such block for the external gate of an exchange-layer op
// (word 0 is the gate), then one ticket line per reconstruction item.
#define CFX_CAP_LINE 16
#define CFX_CAP_GATE_WORDS (25 * CFX_CAP_LINE)
#define CFX_CAP_MAX_ITEMS 16
#define CFX_CAP_TICKET_OFF (2 * CFX_CAP_GATE_WORDS)
#define CFX_CAP_SLOT_WORDS (CFX_CAP_TICKET_OFF + CFX_CAP_MAX_ITEMS * CFX_CAP_LINE)
#define CFX_CAP_MAX_SLOTS 4096        // cfx_set_captured_layer's largest pool: 4096 x 4224 bytes = 16.5 MiB

// the number of the launch that drew `ticket` (an arrival's or an entry ticket's `old`) on a counter that takes `per_launch` of them a launch
CFX_CAP_HD inline cfx_cap_u64 cfx_cap_launch(cfx_cap_u64 ticket, unsigned per_launch) { return ticket / per_launch; }
// whether the arrival that returned `old` completes its launch's n_st: (old + 1) % n_st == 0, written on the dividend of cfx_cap_launch so
// that the device pays for one 64-bit division, not two
CFX_CAP_HD inline bool cfx_cap_last(cfx_cap_u64 old, unsigned n_st) { return old % n_st == n_st - 1u; }
// the value launch r's gates open at: never what launch r - 1 left in the words (all-zero words: launch 0 waits for 1)
CFX_CAP_HD inline unsigned cfx_cap_expect(cfx_cap_u64 r) { return (unsigned)(r + 1); }

#endif
