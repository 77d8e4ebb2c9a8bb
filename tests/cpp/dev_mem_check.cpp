// dev_mem_check.cpp — CPU-only checks of csrc/dev_mem.hpp (the owning device buffers and the device
// guard) against the fake HIP allocator of fake_hip.hpp: malloc-backed, with a map of live blocks, a
// log of every call and a switch that fails the k-th allocation with hipErrorOutOfMemory. Built
// without libamdhip64, with ASan + UBSan (tests/test_dev_mem.py). Exit 0 = every check passed.
#include "fake_hip.hpp"

#include "dev_mem.hpp"

using pvhip::dev_buf;
using pvhip::dev_stream_buf;
using pvhip::device_guard;

static hipStream_t const kStream = (hipStream_t)(uintptr_t)0x51;

// (a) the growth rules ask for exactly their byte counts; (b) a failure empties the buffer
static void check_sync_rules() {
    size_t at = g_log.size();
    dev_buf<uint32_t> b;   // reused scratch: max(n, 1024) elements
    CHECK(b.get() == nullptr && b.capacity() == 0, "a new buffer is empty");
    CHECK(b.grow_floor(0) == hipSuccess && b.get() == nullptr, "nothing asked, nothing allocated");
    CHECK(b.grow_floor(10) == hipSuccess && b.capacity() == 1024 && b.get(), "below the floor");
    EXPECT_CALLS(at, "M4096");
    at = g_log.size();
    const uint32_t* held = b.get();
    CHECK(b.grow_floor(1024) == hipSuccess && b.get() == held, "at capacity");
    EXPECT_CALLS(at, "");
    CHECK(b.grow_floor(1025) == hipSuccess && b.capacity() == 1025, "above capacity");
    EXPECT_CALLS(at, "F4096 M4100");

    at = g_log.size();
    dev_buf<uint8_t> x;   // merge / enc / dec scratch: exactly `need` bytes
    CHECK(x.grow(100, 100) == hipSuccess && x.capacity() == 100, "exact size");
    CHECK(x.grow(100, 100) == hipSuccess && x.grow(7, 7) == hipSuccess, "at and below capacity");
    EXPECT_CALLS(at, "M100");
    CHECK(x.grow(101, 101) == hipSuccess && x.capacity() == 101, "exact regrowth");
    EXPECT_CALLS(at, "M100 F100 M101");

    // the general path's arena: headroom first, then without it, each through grow(); a failed
    // request leaves the buffer empty with capacity 0 and the next one allocates again
    at = g_log.size();
    dev_buf<uint32_t> arena;
    CHECK(arena.grow(800, 900) == hipSuccess && arena.capacity() == 900, "arena with headroom");
    g_fail_in = 1;
    CHECK(arena.grow(1000, 1125) == hipErrorOutOfMemory, "arena out of memory");
    CHECK(arena.get() == nullptr && arena.capacity() == 0, "a failed growth leaves the buffer empty");
    CHECK(arena.grow(1000, 1000) == hipSuccess && arena.get() && arena.capacity() == 1000, "arena without headroom");
    EXPECT_CALLS(at, "M3600 F3600 M4500 M4000");
    arena.release();
    arena.release();   // releasing an empty buffer makes no call
    CHECK(arena.get() == nullptr && arena.capacity() == 0, "released");
    EXPECT_CALLS(at, "M3600 F3600 M4500 M4000 F4000");
}

// (a), (b), (c) for the stream-ordered kind: max(need + need / 8, 64), one retry at max(need, 64)
static void check_stream_rules() {
    size_t at = g_log.size();
    dev_stream_buf<uint64_t> b;
    CHECK(b.grow_headroom(10, kStream) == hipSuccess && b.capacity() == 64, "below the floor");
    EXPECT_CALLS(at, "m512");
    CHECK(b.grow_headroom(64, kStream) == hipSuccess, "at capacity");
    EXPECT_CALLS(at, "m512");
    CHECK(b.grow_headroom(800, kStream) == hipSuccess && b.capacity() == 900, "above capacity");
    EXPECT_CALLS(at, "m512 f512 m7200");
    for (size_t i = at; i < g_log.size(); ++i) CHECK(g_log[i].st == kStream, "call %zu is not on the stream given", i);

    at = g_log.size();
    const int reads = g_err_reads;
    g_fail_in = 1;   // the headroom request fails: the retry asks for `need` itself
    CHECK(b.grow_headroom(8000, kStream) == hipSuccess && b.capacity() == 8000 && b.get(), "retry without headroom");
    EXPECT_CALLS(at, "f7200 m72000 m64000");
    CHECK(g_err_reads == reads + 1, "the sticky error is cleared once before the retry");

    at = g_log.size();
    g_fail_in = 1;
    dev_stream_buf<uint64_t> small;   // ... and the floor holds in the retry
    CHECK(small.grow_headroom(8, kStream) == hipSuccess && small.capacity() == 64, "retry at the floor");
    EXPECT_CALLS(at, "m512 m512");

    at = g_log.size();
    g_fail_in = 1;   // both requests fail
    g_fail_run = 1;
    dev_stream_buf<uint64_t> none;
    CHECK(none.grow_headroom(100, kStream) == hipErrorOutOfMemory, "out of memory twice");
    CHECK(none.get() == nullptr && none.capacity() == 0, "empty after the failure");
    EXPECT_CALLS(at, "m896 m800");
    CHECK(none.grow_headroom(100, kStream) == hipSuccess && none.get() && none.capacity() == 112, "the next call grows again");
    EXPECT_CALLS(at, "m896 m800 m896");

    at = g_log.size();
    dev_stream_buf<uint64_t> sigma;   // chain_set::sigma: exactly slots * sw words
    CHECK(sigma.grow(3 * 128, 3 * 128, kStream) == hipSuccess && sigma.capacity() == 384, "sigma words");
    CHECK(sigma.grow(2 * 128, 2 * 128, kStream) == hipSuccess, "fewer slots");
    EXPECT_CALLS(at, "m3072");
    sigma.release(kStream);
    EXPECT_CALLS(at, "m3072 f3072");
    CHECK(sigma.get() == nullptr && sigma.capacity() == 0, "released on the stream");
    at = g_log.size();
    { dev_stream_buf<uint64_t> left; (void)left.grow(1, 1, kStream); }   // no stream in a destructor: hipFree
    EXPECT_CALLS(at, "m8 F8");
}

// (d) moves leave exactly one owner
static void check_moves() {
    const size_t at = g_log.size();
    {
        dev_buf<uint64_t> a;
        (void)a.grow(5, 5);
        uint64_t* p = a.get();
        dev_buf<uint64_t> b(std::move(a));
        CHECK(a.get() == nullptr && a.capacity() == 0 && b.get() == p && b.capacity() == 5, "move construction");
        dev_buf<uint64_t> c;
        (void)c.grow(9, 9);
        c = std::move(b);   // c's own block goes, b's moves in
        CHECK(b.get() == nullptr && b.capacity() == 0 && c.get() == p && c.capacity() == 5, "move assignment");
        dev_buf<uint64_t>& self = c;
        c = std::move(self);
        CHECK(c.get() == p && c.capacity() == 5, "self move assignment keeps the block");
        dev_stream_buf<uint32_t> s, t;
        (void)s.grow(4, 4, kStream);
        (void)t.grow(6, 6, kStream);
        uint32_t* q = s.get();
        t = std::move(s);
        dev_stream_buf<uint32_t> u(std::move(t));
        CHECK(!s.get() && !t.get() && !s.capacity() && !t.capacity() && u.get() == q && u.capacity() == 4, "stream moves");
        struct four { dev_buf<uint8_t> w, x, y, z; } f;   // a struct of buffers is reset by assignment
        (void)f.w.grow(1, 1);
        (void)f.z.grow(2, 2);
        f = four{};
        CHECK(!f.w.get() && !f.z.get() && !f.z.capacity(), "struct reset");
    }
    EXPECT_CALLS(at, "M40 M72 F72 m16 m24 F24 M1 M2 F1 F2 F16 F40");
    CHECK(g_live.empty(), "%zu blocks still live after the moves", g_live.size());
}

// (e) four arrays grown in sequence, the third allocation failing: each member's capacity matches its
// pointer, so the next call grows exactly what is missing (a chain_set after one out-of-memory)
struct four_arrays {
    dev_stream_buf<uint64_t> meta, w_lo, w_hi, extra;
    hipError_t grow_all(size_t n) {
        for (dev_stream_buf<uint64_t>* b : {&meta, &w_lo, &w_hi, &extra})
            if (const hipError_t e = b->grow(n, n, kStream)) return e;
        return hipSuccess;
    }
};
static void check_partial_failure() {
    four_arrays S;
    CHECK(S.grow_all(100) == hipSuccess, "first growth");
    size_t at = g_log.size();
    g_fail_in = 3;
    CHECK(S.grow_all(200) == hipErrorOutOfMemory, "the third allocation fails");
    EXPECT_CALLS(at, "f800 m1600 f800 m1600 f800 m1600");
    CHECK(S.meta.get() && S.meta.capacity() == 200 && S.w_lo.get() && S.w_lo.capacity() == 200, "grown members");
    CHECK(S.w_hi.get() == nullptr && S.w_hi.capacity() == 0, "the failed member is empty, capacity 0");
    CHECK(S.extra.get() && S.extra.capacity() == 100, "the member not reached keeps its block");
    at = g_log.size();
    CHECK(S.grow_all(200) == hipSuccess, "the next call");
    EXPECT_CALLS(at, "m1600 f800 m1600");
    for (dev_stream_buf<uint64_t>* b : {&S.meta, &S.w_lo, &S.w_hi, &S.extra})
        CHECK(b->get() && b->capacity() == 200, "every member holds 200 after the retry");
    for (dev_stream_buf<uint64_t>* b : {&S.meta, &S.w_lo, &S.w_hi, &S.extra}) b->release(kStream);
}

// (f) the device guard
static int guarded(bool early) {
    device_guard g(5);
    if (g_dev != 5) return -1;
    if (early) return 1;
    g_dev = 6;   // code under the guard may select other devices
    return 0;
}
static void check_device_guard() {
    g_dev = 3;
    CHECK(guarded(false) == 0 && g_dev == 3, "restored on normal exit (device %d)", g_dev);
    CHECK(guarded(true) == 1 && g_dev == 3, "restored on early return (device %d)", g_dev);
    {
        device_guard outer(1);
        { device_guard inner(2); CHECK(g_dev == 2, "inner"); }
        CHECK(g_dev == 1, "nested guards unwind in order");
    }
    CHECK(g_dev == 3, "outer restored");
    g_dev = -1;   // no device to ask for: nothing to put back
    { device_guard g(4); }
    CHECK(g_dev == 4, "no restore when the previous device is unknown");
}

int main() {
    check_sync_rules();
    check_stream_rules();
    check_moves();
    check_partial_failure();
    check_device_guard();
    CHECK(g_live.empty(), "%zu blocks still live at the end", g_live.size());
    if (g_fail) {
        std::fprintf(stderr, "dev_mem_check: %d check(s) failed\n", g_fail);
        return 1;
    }
    std::printf("dev_mem_check: ok (%zu allocator calls)\n", g_log.size());
    return 0;
}
