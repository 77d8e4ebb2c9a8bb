// ctx_check.cpp — CPU-only checks of csrc/ctx.hpp against the fake HIP allocator of fake_hip.hpp: the
// exception boundary of the extern "C" ABI (guarded / caught) and the plan scratch type (begin /
// commit / is_latest / invalidate, and what a failed growth leaves behind). The real header, the host
// side only, without libamdhip64, with ASan + UBSan (tests/test_ctx.py). Exit 0 = every check passed.
#include "fake_hip.hpp"

#include <new>
#include <stdexcept>

#include "ctx.hpp"

using namespace pvhip;

// an entry point as the runtime's units write them: a function-try-block over caught()
static int entry_like(pvac_hip_ctx* c, int what) try {
    if (what == 1) throw std::bad_alloc();
    if (what == 2) throw std::runtime_error("boom");
    if (what == 3) throw 42;   // not a std::exception: nothing to describe
    return fail(c, PVAC_EINVAL, "entry_like: refused");
} catch (...) { return caught(c, "entry_like"); }

static void check_guard() {
    pvac_hip_ctx c;
    c.err = "before";
    CHECK(guarded(&c, "op", [] { return 7; }) == 7 && c.err == "before", "a normal return passes through, err untouched");
    CHECK(guarded(&c, "op", []() -> int { throw std::bad_alloc(); }) == PVAC_ENOMEM, "bad_alloc -> PVAC_ENOMEM");
    CHECK(c.err == std::string("op: ") + std::bad_alloc().what(), "bad_alloc message '%s'", c.err.c_str());
    CHECK(guarded(&c, "set_H", []() -> int { throw std::runtime_error("boom"); }) == PVAC_ENOMEM, "runtime_error -> PVAC_ENOMEM");
    CHECK(c.err == "set_H: boom", "runtime_error message '%s'", c.err.c_str());
    // without a context: the same codes, nothing to write to
    CHECK(guarded(nullptr, "op", [] { return 0; }) == 0, "normal return, null context");
    CHECK(guarded(nullptr, "op", []() -> int { throw std::bad_alloc(); }) == PVAC_ENOMEM, "bad_alloc, null context");
    CHECK(guarded(nullptr, "op", []() -> int { throw std::runtime_error("x"); }) == PVAC_ENOMEM, "runtime_error, null context");
    // the entries' own shape
    CHECK(entry_like(&c, 0) == PVAC_EINVAL && c.err == "entry_like: refused", "an entry's own failure passes through");
    CHECK(entry_like(&c, 1) == PVAC_ENOMEM && c.err == std::string("entry_like: ") + std::bad_alloc().what(), "entry, bad_alloc");
    CHECK(entry_like(&c, 2) == PVAC_ENOMEM && c.err == "entry_like: boom", "entry, runtime_error");
    CHECK(entry_like(nullptr, 1) == PVAC_ENOMEM && entry_like(nullptr, 2) == PVAC_ENOMEM, "entry, null context");
    CHECK(entry_like(&c, 3) == PVAC_ENOMEM && c.err.empty(), "any other exception stays inside too");
    CHECK(entry_like(nullptr, 3) == PVAC_ENOMEM, "... also without a context");
}

static pvac_hip_plan committed(plan_scratch& ps) {
    pvac_hip_plan p{};
    ps.commit(&p);
    return p;
}

static void check_stamps() {
    plan_scratch ps;
    CHECK(ps.init() == hipSuccess && ps.totals && ps.capacity() == 0, "init");
    const pvac_hip_plan never{};   // a plan no plan pass has committed
    CHECK(!ps.is_latest(&never), "an uncommitted plan is not latest on a new context");
    CHECK(ps.begin(10) == hipSuccess && ps.capacity() == 1024, "first begin: the floor of 1,024 pairs");
    const pvac_hip_plan p1 = committed(ps);
    CHECK(ps.is_latest(&p1) && !ps.is_latest(&never), "the committed plan is latest, the uncommitted one is not");
    // begin without growth: same arrays, new stamp
    const size_t at = g_log.size();
    const uint8_t* held = ps.pair_class.get();
    CHECK(ps.begin(1024) == hipSuccess && ps.pair_class.get() == held, "begin at capacity keeps the arrays");
    EXPECT_CALLS(at, "");
    CHECK(!ps.is_latest(&p1), "a plan committed before a later begin is not latest (no growth)");
    CHECK(!ps.is_latest(&never), "uncommitted, after a begin nobody committed");
    const pvac_hip_plan p2 = committed(ps);
    CHECK(p2.reserved[0] != p1.reserved[0] && ps.is_latest(&p2), "begin changed the stamp");
    // begin with growth
    CHECK(ps.begin(1025) == hipSuccess && ps.capacity() == 1025, "begin above capacity grows");
    CHECK(!ps.is_latest(&p2) && !ps.is_latest(&p1), "a plan committed before a later begin is not latest (growth)");
    const pvac_hip_plan p3 = committed(ps);
    CHECK(p3.reserved[0] != p2.reserved[0] && p3.reserved[0] != p1.reserved[0] && ps.is_latest(&p3), "begin changed the stamp again");
    // the explicit invalidation (a failed redo, a failed re-group, a capacity check)
    ps.invalidate();
    CHECK(!ps.is_latest(&p3) && !ps.is_latest(&never), "invalidate leaves no plan latest");
    // begin(0) is a plan too
    CHECK(ps.begin(0) == hipSuccess, "begin(0)");
    const pvac_hip_plan p4 = committed(ps);
    CHECK(ps.is_latest(&p4) && p4.reserved[0] != p3.reserved[0] && p4.reserved[0] != 0, "begin(0) takes a stamp");
}

// the k-th allocation of a growth fails, for each k: capacity 0, everything it took given back (the
// stats record, which no growth takes, stays), the plan before it stale, and the next begin succeeds
static void check_failed_growth() {
    for (int first = 0; first < 2; ++first) {   // 1: the context's first growth (redo_cnt is allocated too)
        const int allocs = first ? 7 : 6;
        for (int k = 1; k <= allocs; ++k) {
            plan_scratch ps;
            CHECK(ps.init() == hipSuccess, "init");
            pvac_hip_plan before{};
            if (!first) {
                CHECK(ps.begin(100) == hipSuccess, "a first begin");
                before = committed(ps);
                ps.redo_cnt_dirty = false;   // as after an exec that read back a zero count
            }
            const size_t at = g_log.size();
            g_fail_in = k;
            CHECK(ps.begin(5000) == hipErrorOutOfMemory, "first %d, k %d: begin reports the failure", first, k);
            CHECK(g_fail_in == 0, "first %d, k %d: the growth made at least k allocations", first, k);
            CHECK(ps.capacity() == 0, "first %d, k %d: capacity 0 after the failure", first, k);
            CHECK(g_live.size() == 1 && g_live.begin()->first == (void*)ps.stats.get(),
                  "first %d, k %d: %zu blocks live after the failure (calls '%s')", first, k, g_live.size(), calls_since(at).c_str());
            CHECK(!ps.pair_class.get() && !ps.pair_status.get() && !ps.large_ids.get() && !ps.large_info.get() &&
                      !ps.fresh_recs.get() && !ps.redo_ids.get() && !ps.redo_cnt.get(),
                  "first %d, k %d: no array keeps a pointer", first, k);
            CHECK(ps.redo_cnt_dirty, "first %d, k %d: a redo count allocated anew is not known to be zero", first, k);
            CHECK(!ps.is_latest(&before), "first %d, k %d: the failed begin still made the earlier plan stale", first, k);
            CHECK(ps.begin(5000) == hipSuccess && ps.capacity() == 5000, "first %d, k %d: the next begin succeeds", first, k);
            CHECK(ps.pair_class.capacity() == 5000 && ps.pair_status.capacity() == 5000 && ps.large_ids.capacity() == 5000 &&
                      ps.large_info.capacity() == 8 * 5000 && ps.fresh_recs.capacity() == 5000 && ps.redo_cnt.capacity() == 4,
                  "first %d, k %d: every array holds the new batch", first, k);
            const pvac_hip_plan after = committed(ps);
            CHECK(ps.is_latest(&after) && !ps.is_latest(&before), "first %d, k %d: the new plan is latest", first, k);
        }
    }
    CHECK(g_live.empty(), "%zu blocks still live after the scratch went", g_live.size());
}

int main() {
    check_guard();
    check_stamps();
    check_failed_growth();
    CHECK(g_live.empty(), "%zu blocks still live at the end", g_live.size());
    if (g_fail) {
        std::fprintf(stderr, "ctx_check: %d check(s) failed\n", g_fail);
        return 1;
    }
    std::printf("ctx_check: ok (%zu allocator calls)\n", g_log.size());
    return 0;
}
