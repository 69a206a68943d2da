// Host check of frieda_amd/csrc/unit_pipeline.h: the order in which a device's worker uploads, begins, finishes and abandons its
// units (run_unit_pass) and the retry of a pass that ran out of device memory (run_unit_passes), under recording fakes.  Whole traces
// are compared: U = upload, B = begin, F = finish, A = abandon, each with its unit's index, "✗" behind a call that failed.
#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "unit_pipeline.h"

using namespace frieda;

static long bad = 0;
static void expect(bool ok, const char* name, const std::string& got) {
    if (ok) return;
    printf("%s: got %s\n", name, got.c_str());
    bad++;
}

// the share starts at slot 5 (as after a retry) and the units differ in size: `done` is told apart from a unit's index
static const std::vector<Unit> kUnits = {{5, 1}, {6, 2}, {8, 3}, {11, 2}};
static uint32_t end_of(size_t u) { return kUnits[u].slot + kUnits[u].cnt; }

struct Fakes {
    std::vector<Unit> units;
    bool prefetch = true;
    std::atomic<bool> abort{false};
    std::map<std::string, int> failing;  // "B2" -> the status that call returns
    std::string trace, err, what;
    uint32_t done = 5;

    int call(char kind, size_t u) {
        const std::string name = kind + std::to_string(u);
        trace += (trace.empty() ? "" : " ") + name;
        const auto f = failing.find(name);
        if (f == failing.end()) return FRIEDA_OK;
        trace += "✗";
        err = name + " failed";
        return f->second;
    }
    int pass(const std::vector<Unit>& us, uint32_t& d) {
        return run_unit_pass(
            us, prefetch, abort, [&](size_t u) { return call('U', u); }, [&](size_t u) { return call('B', u); },
            [&](size_t u) { return call('F', u); }, [&](size_t u) { (void)call('A', u); }, d, err, what);
    }
};

// one pass over the first n_units of kUnits: the trace, the status, `done` and the text of the first failure
static void pass_case(const char* name, size_t n_units, bool prefetch, bool abort, std::map<std::string, int> failing, const char* trace,
                      int status, uint32_t done, const char* what = "") {
    Fakes f;
    f.units.assign(kUnits.begin(), kUnits.begin() + n_units);
    f.prefetch = prefetch;
    f.abort.store(abort);
    f.failing = std::move(failing);
    const int st = f.pass(f.units, f.done);
    expect(f.trace == trace, name, f.trace);
    expect(st == status, name, "status " + std::to_string(st));
    expect(f.done == done, name, "done " + std::to_string(f.done));
    expect(f.what == what, name, "what '" + f.what + "'");
}

// the retry loop over a scripted pass: every cut's (from_slot, shrink), the drops, the passes run.  A cut returns the units that end
// behind from_slot.
struct Passes {
    std::vector<Unit> units, left;
    std::atomic<bool> abort{false};
    std::vector<std::pair<uint32_t, uint32_t>> cuts;
    int drops = 0, prepares = 0, passes = 0;

    template <class Prepare, class Pass>
    int run(Prepare&& prepare, Pass&& pass) {
        return run_unit_passes(
            abort,
            [&](uint32_t from, uint32_t shrink) -> const std::vector<Unit>& {
                cuts.push_back({from, shrink});
                left.clear();
                for (const Unit& un : units)
                    if (un.slot + un.cnt > from) left.push_back(un);
                return left;
            },
            [&] {
                prepares++;
                return prepare();
            },
            [&] { drops++; },
            [&](const std::vector<Unit>& us, uint32_t& done) {
                passes++;
                return pass(us, done);
            });
    }
};
static int prepared() { return FRIEDA_OK; }

int main() {
    const int NOMEM = FRIEDA_ERR_NOMEM, HIP = FRIEDA_ERR_HIP;
    pass_case("1: 1 unit, prefetch", 1, true, false, {}, "U0 B0 F0", FRIEDA_OK, end_of(0));
    pass_case("2: 3 units, prefetch", 3, true, false, {}, "U0 U1 B0 B1 U2 F0 B2 F1 F2", FRIEDA_OK, end_of(2));
    pass_case("3: 4 units, prefetch", 4, true, false, {}, "U0 U1 B0 B1 U2 F0 B2 U3 F1 B3 F2 F3", FRIEDA_OK, end_of(3));
    pass_case("4: 4 units, no prefetch", 4, false, false, {}, "B0 B1 F0 B2 F1 B3 F2 F3", FRIEDA_OK, end_of(3));
    pass_case("5: upload(1) fails", 3, true, false, {{"U1", HIP}}, "U0 U1✗", HIP, 5, "U1 failed");
    pass_case("6: begin(0) fails", 3, true, false, {{"B0", HIP}}, "U0 U1 B0✗", HIP, 5, "B0 failed");
    pass_case("7: begin(2) fails with NOMEM", 3, true, false, {{"B2", NOMEM}}, "U0 U1 B0 B1 U2 F0 B2✗ F1", NOMEM, end_of(1), "B2 failed");
    pass_case("8: finish(0) fails", 3, true, false, {{"F0", HIP}}, "U0 U1 B0 B1 U2 F0✗ A1", HIP, 5, "F0 failed");
    pass_case("9: begin(1) fails with NOMEM, finish(0) with HIP", 3, true, false, {{"B1", NOMEM}, {"F0", HIP}}, "U0 U1 B0 B1✗ U2 F0✗", NOMEM, 5,
              "B1 failed");
    pass_case("10: abort already set", 3, true, true, {}, "U0 U1 B0 F0", FRIEDA_OK, end_of(0));
    pass_case("no units", 0, true, false, {}, "", FRIEDA_OK, 5);

    {  // 11: NOMEM on every pass (each finishing one more blob), a unit of more than one blob: 17 cuts with shrink 0 .. 16, 16 drops
        Passes p;
        p.units = {{0, 100}};
        const int st = p.run(prepared, [](const std::vector<Unit>&, uint32_t& done) {
            done++;
            return FRIEDA_ERR_NOMEM;
        });
        bool cuts_ok = p.cuts.size() == 17;
        for (uint32_t k = 0; k < p.cuts.size(); k++) cuts_ok = cuts_ok && p.cuts[k] == std::make_pair(k, k);  // from the current `done`
        expect(cuts_ok && p.drops == 16 && p.passes == 17 && st == NOMEM, "11: NOMEM on every pass",
               std::to_string(p.cuts.size()) + " cuts, " + std::to_string(p.drops) + " drops, status " + std::to_string(st));
    }
    {  // 12: NOMEM where every unit is a single blob: halving cannot help
        Passes p;
        p.units = {{0, 1}, {1, 1}, {2, 1}};
        const int st = p.run(prepared, [](const std::vector<Unit>&, uint32_t&) { return FRIEDA_ERR_NOMEM; });
        expect(p.cuts.size() == 1 && p.passes == 1 && p.drops == 0 && st == NOMEM, "12: NOMEM, single blobs", std::to_string(p.drops) + " drops");
    }
    {  // 13: another error is not retried
        Passes p;
        p.units = kUnits;
        const int st = p.run(prepared, [](const std::vector<Unit>&, uint32_t&) { return FRIEDA_ERR_HIP; });
        expect(p.cuts.size() == 1 && p.passes == 1 && p.drops == 0 && st == HIP, "13: FRIEDA_ERR_HIP", std::to_string(p.drops) + " drops");
    }
    {  // 14: NOMEM while another device has failed
        Passes p;
        p.units = kUnits;
        p.abort.store(true);
        const int st = p.run(prepared, [](const std::vector<Unit>&, uint32_t&) { return FRIEDA_ERR_NOMEM; });
        expect(p.cuts.size() == 1 && p.passes == 1 && p.drops == 0 && st == NOMEM, "14: NOMEM with abort set", std::to_string(p.drops) + " drops");
    }
    {  // 15: the real pass; NOMEM on the first one after unit 0 finished, then success over the two units left
        Passes p;
        p.units = {{0, 1}, {1, 2}, {3, 3}};
        Fakes f;
        f.failing = {{"B1", NOMEM}};
        uint32_t first_done = 0;
        const int st = p.run(prepared, [&](const std::vector<Unit>& us, uint32_t& done) {
            const int rc = f.pass(us, done);
            if (p.passes == 1) first_done = done;
            f.failing.clear();
            return rc;
        });
        expect(f.trace == "U0 U1 B0 B1✗ U2 F0 U0 U1 B0 B1 F0 F1", "15: trace", f.trace);
        expect(first_done == 1 && p.cuts.size() == 2 && p.cuts[0] == std::make_pair(0u, 0u) && p.cuts[1] == std::make_pair(first_done, 1u) &&
                   p.drops == 1 && p.passes == 2 && st == FRIEDA_OK,
               "15: NOMEM, then success", std::to_string(p.cuts.size()) + " cuts, status " + std::to_string(st));
    }
    {  // an empty cut ends the loop before anything is prepared; a prepare that runs out of memory counts as its pass
        Passes p;
        const int st = p.run(prepared, [](const std::vector<Unit>&, uint32_t&) { return FRIEDA_ERR_HIP; });
        expect(p.cuts.size() == 1 && p.prepares == 0 && p.passes == 0 && st == FRIEDA_OK, "empty cut", "status " + std::to_string(st));
        Passes q;
        q.units = kUnits;
        int asked = 0;
        const int sq = q.run([&] { return asked++ == 0 ? FRIEDA_ERR_NOMEM : FRIEDA_OK; },
                             [](const std::vector<Unit>& us, uint32_t& done) {
                                 done = us.back().slot + us.back().cnt;
                                 return FRIEDA_ERR_HIP;
                             });
        expect(q.cuts.size() == 2 && q.cuts[1] == std::make_pair(0u, 1u) && q.drops == 1 && q.passes == 1 && sq == HIP, "prepare NOMEM",
               std::to_string(q.cuts.size()) + " cuts, status " + std::to_string(sq));
    }
    if (bad) {
        printf("FAILED: %ld\n", bad);
        return 1;
    }
    printf("OK\n");
    return 0;
}
