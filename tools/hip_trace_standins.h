// Stand-ins for the slice of the HIP runtime that a compiled .hip object of csrc/ uses, so that such objects link into
// a plain program and their host side runs without a GPU (tools/jacobi_dispatch_trace.cpp,
// tools/procrustes_dispatch_trace.cpp, tools/tridiag_dispatch_trace.cpp).  The stand-ins launch nothing: they record the
// kernel name, grid, block and dynamic LDS bytes of every launch, every function attribute that is set, the byte count
// of every fill / copy and every event that is recorded.
// Runs of identical consecutive records (the rounds of a block solver) are folded into one line with a count.
// Include once, in the one translation unit of the tracer.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cxxabi.h>
#include <map>
#include <set>
#include <string>

// ---- the slice of the HIP ABI that a compiled .hip object uses --------------------------------------------------
#include "../include/basd_hip.h"     // the entry points under test, and hipStream_t
struct dim3 { uint32_t x, y, z; };

static std::map<const void*, std::string> g_kernels;   // host stub -> demangled kernel name
static std::string g_seq, g_last;                       // launch sequence of the current call; its last line
static long g_repeat = 0;
static struct { dim3 grid, block; size_t lds; hipStream_t stream; } g_config;

static void flush_last() {
    if (g_last.empty()) return;
    g_seq += "  " + g_last;
    if (g_repeat > 1) g_seq += " x" + std::to_string(g_repeat);
    g_seq += "\n";
    g_last.clear();
    g_repeat = 0;
}
static void record(const std::string& line) {
    if (line == g_last) { ++g_repeat; return; }
    flush_last();
    g_last = line;
    g_repeat = 1;
}
static std::string kernel_name(const void* f) {
    auto it = g_kernels.find(f);
    return it == g_kernels.end() ? "<unregistered>" : it->second;
}

static long g_calls = 0;
static std::set<std::string> g_distinct;

// end of one call under test: print its heading, status and launch sequence
static void finish_call(const char* what, int rc) {
    flush_last();
    printf("%s rc=%d\n%s", what, rc, g_seq.c_str());
    ++g_calls;
    g_distinct.insert(g_seq);
    g_seq.clear();
}

extern "C" {
void** __hipRegisterFatBinary(const void*) { static void* handle; return &handle; }
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterFunction(void**, const void* host_fn, char*, const char* device_name, unsigned, void*, void*, void*,
                           void*, int*) {
    int status = 0;
    char* d = abi::__cxa_demangle(device_name, nullptr, nullptr, &status);
    std::string name = status == 0 && d ? d : device_name;
    free(d);
    const size_t paren = name.find('(');                // keep name and template arguments, drop the parameter list
    if (paren != std::string::npos) name.resize(paren);
    if (name.rfind("void ", 0) == 0) name.erase(0, 5);
    g_kernels[host_fn] = name;
}
int __hipPushCallConfiguration(dim3 grid, dim3 block, size_t lds, hipStream_t stream) {
    g_config = {grid, block, lds, stream};
    return 0;
}
int __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* lds, hipStream_t* stream) {
    *grid = g_config.grid; *block = g_config.block; *lds = g_config.lds; *stream = g_config.stream;
    return 0;
}
int hipLaunchKernel(const void* f, dim3 grid, dim3 block, void**, size_t lds, hipStream_t) {
    char buf[160];
    snprintf(buf, sizeof buf, " grid=%u,%u,%u block=%u,%u,%u lds=%zu", grid.x, grid.y, grid.z, block.x, block.y, block.z, lds);
    record("launch " + kernel_name(f) + buf);
    return 0;
}
int hipFuncSetAttribute(const void* f, int attr, int value) {
    record("attr " + kernel_name(f) + " " + std::to_string(attr) + "=" + std::to_string(value));
    return 0;
}
int hipGetLastError(void) { return 0; }
int hipMemsetAsync(void*, int value, size_t bytes, hipStream_t) {
    record("memset value=" + std::to_string(value) + " bytes=" + std::to_string(bytes));
    return 0;
}
int hipMemcpyAsync(void*, const void*, size_t bytes, int kind, hipStream_t) {
    record("memcpy kind=" + std::to_string(kind) + " bytes=" + std::to_string(bytes));
    return 0;
}
// the device that occupancy-sized launches see: 256 CUs, one workgroup of any kernel per CU
int hipGetDevice(int* device) { *device = 0; return 0; }
int hipDeviceGetAttribute(int* value, int, int) { *value = 256; return 0; }
int hipOccupancyMaxActiveBlocksPerMultiprocessor(int* blocks, const void*, int, size_t) { *blocks = 1; return 0; }
int hipEventRecord(void*, hipStream_t) { record("event record"); return 0; }
int hipEventCreateWithFlags(void**, unsigned) { return 0; }
int hipEventDestroy(void*) { return 0; }
int hipStreamWaitEvent(hipStream_t, void*, unsigned) { return 0; }
}  // extern "C"
