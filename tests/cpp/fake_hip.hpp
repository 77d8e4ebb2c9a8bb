// fake_hip.hpp — a fake HIP allocator for the CPU-only checks of the runtime's host code
// (dev_mem_check.cpp, ctx_check.cpp): malloc-backed, with a map of live blocks, a log of every call
// and a switch that fails the k-th allocation with hipErrorOutOfMemory. It defines the runtime's
// allocation and device-selection entry points itself, so a check links without libamdhip64.
// Include it once, in the check's only translation unit.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

static int g_fail = 0;
#define CHECK(c, ...)                                   \
    do {                                                \
        if (!(c)) {                                     \
            std::fprintf(stderr, "FAIL %d: ", __LINE__); \
            std::fprintf(stderr, __VA_ARGS__);          \
            std::fprintf(stderr, "\n");                 \
            ++g_fail;                                   \
        }                                               \
    } while (0)

struct call {
    char kind;   // 'M' hipMalloc, 'F' hipFree, 'm' hipMallocAsync, 'f' hipFreeAsync
    size_t bytes;
    hipStream_t st;
};
static std::map<void*, size_t> g_live;
static std::vector<call> g_log;
static int g_fail_in = 0;       // > 0: the g_fail_in-th allocation from now fails ...
static int g_fail_run = 0;      // ... and so do the g_fail_run allocations after it
static int g_err_reads = 0;     // hipGetLastError calls
static int g_dev = 0;           // the selected device; < 0: hipGetDevice fails (no GPU)

static hipError_t fake_alloc(void** p, size_t bytes, char kind, hipStream_t st) {
    g_log.push_back({kind, bytes, st});
    if ((g_fail_in > 0 && --g_fail_in == 0) || (g_fail_in == 0 && g_fail_run > 0 && g_fail_run--)) {
        *p = (void*)(uintptr_t)0xBAD;   // a failed allocation's output must not be kept
        return hipErrorOutOfMemory;
    }
    CHECK(bytes > 0, "allocation of 0 bytes");
    *p = std::malloc(bytes);
    g_live[*p] = bytes;
    return hipSuccess;
}
static hipError_t fake_free(void* p, char kind, hipStream_t st) {
    auto it = g_live.find(p);
    CHECK(it != g_live.end(), "free of %p, which is not a live block", p);
    if (it == g_live.end()) return hipErrorInvalidValue;
    g_log.push_back({kind, it->second, st});
    g_live.erase(it);
    std::free(p);
    return hipSuccess;
}
extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) { return fake_alloc(p, bytes, 'M', nullptr); }
hipError_t hipFree(void* p) { return fake_free(p, 'F', nullptr); }
hipError_t hipMallocAsync(void** p, size_t bytes, hipStream_t st) { return fake_alloc(p, bytes, 'm', st); }
hipError_t hipFreeAsync(void* p, hipStream_t st) { return fake_free(p, 'f', st); }
hipError_t hipGetLastError(void) { ++g_err_reads; return hipSuccess; }
hipError_t hipSetDevice(int d) { g_dev = d; return hipSuccess; }
hipError_t hipGetDevice(int* d) {
    if (g_dev < 0) return hipErrorNoDevice;
    *d = g_dev;
    return hipSuccess;
}
}

// the calls logged since `from` as text, e.g. "F4096 M8200"
static std::string calls_since(size_t from) {
    std::string s;
    for (size_t i = from; i < g_log.size(); ++i)
        s += (s.empty() ? "" : " ") + std::string(1, g_log[i].kind) + std::to_string(g_log[i].bytes);
    return s;
}
#define EXPECT_CALLS(from, want) CHECK(calls_since(from) == (want), "calls '%s', expected '%s'", calls_since(from).c_str(), want)
