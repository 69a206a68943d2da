// unit_pipeline.h — the order in which one device's worker (multi.cpp) uploads, begins and finishes its units, and the retry of a
// pass that ran out of device memory.  No HIP, no contexts: the four operations are passed in, so the order — the part a mistake
// turns into a ring slot overwritten while a kernel still reads it, or a context left with a job in flight — runs on the CPU under
// recording fakes (tests/cpp/test_unit_pipeline.cpp).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <string>
#include <vector>

#include "../../include/frieda_hip.h"  // the status codes

namespace frieda {

// `cnt` consecutive blobs of a device's share, from its `slot`-th: one call of the batched kernels
struct Unit {
    uint32_t slot, cnt;
};

// One pass over `units`: two units in flight (on the two contexts of the device) and, when `prefetch`, the blobs of the unit after
// them on their way into the upload ring (three slots: unit u + 2 takes the slot of unit u - 1, which has finished).
//   upload(u), begin(u), finish(u) -> status;  abandon(u): finish a begun unit for nobody, the context must stay usable.
// A callable that fails leaves its text in `err`.  The first error is the pass's status and `what`; later ones are dropped.  `done`
// advances to the end of every unit that finished.  After an error, or once `abort` is set (another device failed), nothing more is
// begun: the unit in flight is finished, the one begun after it abandoned.
template <class Upload, class Begin, class Finish, class Abandon>
int run_unit_pass(const std::vector<Unit>& units, bool prefetch, const std::atomic<bool>& abort, Upload&& upload, Begin&& begin,
                  Finish&& finish, Abandon&& abandon, uint32_t& done, const std::string& err, std::string& what) {
    int st = FRIEDA_OK;
    auto bail = [&](int rc) {
        if (rc != FRIEDA_OK && st == FRIEDA_OK) {
            st = rc;
            what = err;
        }
        return rc;
    };
    if (units.empty()) return st;
    for (size_t u = 0; prefetch && u < 2 && u < units.size(); u++)
        if (bail(upload(u)) != FRIEDA_OK) return st;
    if (bail(begin(0)) != FRIEDA_OK) return st;
    for (size_t u = 0; u < units.size(); u++) {
        bool next_begun = false;
        if (u + 1 < units.size() && !abort.load()) next_begun = bail(begin(u + 1)) == FRIEDA_OK;
        if (prefetch && u + 2 < units.size() && !abort.load()) bail(upload(u + 2));
        if (bail(finish(u)) == FRIEDA_OK) done = units[u].slot + units[u].cnt;
        if (st != FRIEDA_OK || abort.load()) {
            if (next_begun) abandon(u + 1);
            break;
        }
    }
    return st;
}

// The passes over a device's share.  A pass that ran out of device memory is repeated from the first blob not yet done with the calls
// halved once more, while halving can still make a call smaller.
//   cut(from_slot, shrink) -> const std::vector<Unit>&: what is left, as units (empty: nothing is);
//   prepare() -> status: what those units need before the first upload;  drop(): free the device's workspaces before a retry;
//   pass(units, done) -> status: run_unit_pass over the caller's operations.
template <class Cut, class Prepare, class Drop, class Pass>
int run_unit_passes(const std::atomic<bool>& abort, Cut&& cut, Prepare&& prepare, Drop&& drop, Pass&& pass) {
    uint32_t done = 0;
    for (uint32_t shrink = 0;; shrink++) {
        const std::vector<Unit>& units = cut(done, shrink);
        if (units.empty()) return FRIEDA_OK;
        uint32_t largest = 1;
        for (const Unit& un : units) largest = std::max(largest, un.cnt);
        int st = prepare();
        if (st == FRIEDA_OK) st = pass(units, done);
        if (!(st == FRIEDA_ERR_NOMEM && largest > 1 && !abort.load() && shrink < 16)) return st;
        drop();
    }
}

}  // namespace frieda
