// A host-only stand-in for <hip/hip_runtime.h>, for tests/devmem_host.cpp: the runtime calls fb_devmem.h
// makes, and nothing else.  Allocations sit over malloc with a set of the live ones -- freeing a pointer that
// is not in it aborts -- and a switch makes the k-th allocation from now fail; every event and stream call,
// and every allocation and free, is appended to a call log the test reads.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <vector>

typedef int hipError_t;
enum { hipSuccess = 0, hipErrorOutOfMemory = 2 };
typedef struct stub_event* hipEvent_t;
typedef struct stub_stream* hipStream_t;
enum { hipHostMallocDefault = 0u, hipHostMallocMapped = 2u, hipEventDisableTiming = 2u, hipStreamNonBlocking = 1u };

namespace hipstub {
struct Call {
    std::string fn;
    const void *a, *b;  // the call's object and its stream / second object
    bool operator==(const Call& o) const { return fn == o.fn && a == o.a && b == o.b; }
};
inline std::vector<Call>& log() { static std::vector<Call> v; return v; }
inline std::set<void*>& live() { static std::set<void*> s; return s; }
inline int& fail_in() { static int k = 0; return k; }  // k > 0: the k-th allocation from now fails
inline void note(const char* fn, const void* a = nullptr, const void* b = nullptr) { log().push_back({fn, a, b}); }
inline hipError_t alloc(const char* fn, void** p, size_t bytes) {
    if (fail_in() > 0 && --fail_in() == 0) {
        note("alloc-failed");
        *p = reinterpret_cast<void*>(0xBAD);  // (a failed call's output must not be trusted)
        return hipErrorOutOfMemory;
    }
    *p = malloc(bytes ? bytes : 1);
    live().insert(*p);
    note(fn, *p);
    return hipSuccess;
}
inline hipError_t release(const char* fn, void* p) {
    if (!live().erase(p)) {
        fprintf(stderr, "hipstub: %s(%p): not a live allocation\n", fn, p);
        abort();
    }
    note(fn, p);
    free(p);
    return hipSuccess;
}
template <class T>
hipError_t make(const char* fn, T** out) {
    void* p = malloc(1);  // (an event or a stream: live like an allocation, never made to fail)
    live().insert(p);
    note(fn, p);
    *out = static_cast<T*>(p);
    return hipSuccess;
}
}  // namespace hipstub

inline hipError_t hipMalloc(void** p, size_t bytes) { return hipstub::alloc("hipMalloc", p, bytes); }
inline hipError_t hipFree(void* p) { return hipstub::release("hipFree", p); }
inline hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) { return hipstub::alloc("hipHostMalloc", p, bytes); }
inline hipError_t hipHostFree(void* p) { return hipstub::release("hipHostFree", p); }
inline hipError_t hipHostGetDevicePointer(void** d, void* h, unsigned) { *d = h; return hipSuccess; }
inline hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return hipstub::make("hipEventCreate", e); }
inline hipError_t hipEventDestroy(hipEvent_t e) { return hipstub::release("hipEventDestroy", e); }
inline hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) { hipstub::note("hipEventRecord", e, s); return hipSuccess; }
inline hipError_t hipEventSynchronize(hipEvent_t e) { hipstub::note("hipEventSynchronize", e); return hipSuccess; }
inline hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) { hipstub::note("hipStreamWaitEvent", e, s); return hipSuccess; }
inline hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { return hipstub::make("hipStreamCreate", s); }
inline hipError_t hipStreamDestroy(hipStream_t s) { return hipstub::release("hipStreamDestroy", s); }
inline const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "out of memory"; }
