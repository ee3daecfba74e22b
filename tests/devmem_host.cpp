// Stand-alone host check of flodbadd_amd/csrc/fb_devmem.h (the real header) over tests/hipstub's runtime:
//   g++ -std=c++17 -fsanitize=address,undefined -I tests/hipstub tests/devmem_host.cpp
// Exits non-zero at the first miss; the leak check stays on, and the stub aborts on a double free.
#include <cstdarg>

#include "../flodbadd_amd/csrc/fb_devmem.h"

using namespace fbk;
using hipstub::Call;

static char g_err[256];
int fbk::set_err(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define CHECK(x)                                                       \
    do {                                                               \
        if (!(x)) {                                                    \
            fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #x); \
            exit(1);                                                   \
        }                                                              \
    } while (0)

static size_t count(const char* fn, size_t from = 0) {
    size_t n = 0;
    for (size_t i = from; i < hipstub::log().size(); ++i) n += hipstub::log()[i].fn == fn;
    return n;
}
static bool nothing_live() { return hipstub::live().empty(); }

static void test_devbuf() {
    {
        DevBuf<int> b;
        CHECK(!b && b.size() == 0);
        CHECK(b.alloc(10) == hipSuccess && b.get() && b.size() == 10 && hipstub::live().count(b.get()));
        int* first = b.get();
        const size_t at = hipstub::log().size();
        CHECK(b.alloc(20) == hipSuccess && b.size() == 20);  // the old block goes first
        CHECK(hipstub::log().size() == at + 2 && (hipstub::log()[at] == Call{"hipFree", first, nullptr}) &&
              (hipstub::log()[at + 1] == Call{"hipMalloc", b.get(), nullptr}));
        CHECK(hipstub::live().size() == 1);
        CHECK(b.alloc(0) == hipSuccess && !b.get() && b.size() == 0 && nothing_live());  // empty, and a success
        CHECK(b.alloc(5) == hipSuccess);
        hipstub::fail_in() = 1;
        CHECK(b.alloc(7) != hipSuccess && !b.get() && b.size() == 0 && nothing_live());  // a failure leaves it empty
        CHECK(b.alloc(3) == hipSuccess);
        int* p = b.get();
        DevBuf<int> c(std::move(b));  // move: c owns it, b is empty
        CHECK(c.get() == p && c.size() == 3 && !b.get() && b.size() == 0);
        DevBuf<int> d;
        CHECK(d.alloc(4) == hipSuccess);
        int* q = d.get();
        c.swap(d);
        CHECK(c.get() == q && c.size() == 4 && d.get() == p && d.size() == 3);
        d = std::move(c);  // move assignment: what d held is freed at once, c is left empty
        CHECK(d.get() == q && !c.get() && hipstub::live().count(q) && !hipstub::live().count(p));
        d.reset();
        CHECK(!d.get() && nothing_live());
        d.reset();  // (twice is fine)
        PinnedBuf<long> h;
        CHECK(h.alloc(8, hipHostMallocMapped) == hipSuccess && h.dev() == h.get() && h.size() == 8);
        CHECK(h.alloc(2, hipHostMallocDefault) == hipSuccess && h.dev() == nullptr);
        CHECK(count("hipHostFree") == 1);
        PinnedBuf<long> g(std::move(h));
        CHECK(g.get() && !h.get());
    }
    CHECK(nothing_live());
    CHECK(count("hipHostFree") == 2 && count("hipHostMalloc") == 2);
}

struct Group4 {
    DevBuf<char> a;
    DevBuf<int> b;
    DevBuf<double> c;
    DevBuf<short> d;
    int cap = 0;
};
static hipError_t fill(Group4& g) {
    return alloc_group(g, [](Group4& n) {
        n.cap = 9;
        return alloc_each(n.a, 1, n.b, 2, n.c, 3, n.d, 4);
    });
}
static void test_group() {
    {
        Group4 g;
        for (int k = 1; k <= 4; ++k) {
            hipstub::fail_in() = k;
            CHECK(fill(g) != hipSuccess);
            CHECK(!g.a && !g.b && !g.c && !g.d && g.cap == 0 && nothing_live());
            CHECK(hipstub::fail_in() == 0);
        }
        CHECK(fill(g) == hipSuccess && g.a.size() == 1 && g.b.size() == 2 && g.c.size() == 3 && g.d.size() == 4 && g.cap == 9);
        hipstub::fail_in() = 3;  // a failed re-allocation drops the group it held, too
        CHECK(fill(g) != hipSuccess && !g.a && !g.d && g.cap == 0 && nothing_live());
        CHECK(fill(g) == hipSuccess && hipstub::live().size() == 4);
        g = Group4();  // dropped by assignment of an empty value
        CHECK(nothing_live());
        CHECK(fill(g) == hipSuccess);
    }
    CHECK(nothing_live());
}

static void test_scratch() {
    const hipStream_t sa = reinterpret_cast<hipStream_t>(0x100), sb = reinterpret_cast<hipStream_t>(0x200);
    const size_t t0 = hipstub::log().size();
    {
        StreamScratch s;
        CHECK(count("hipEventCreate", t0) == 0 && s.get() == nullptr && s.capacity() == 0);
        // the first acquire: the event is made, the stream waits for it, and the growth is sync, (free,) allocate
        CHECK(s.acquire(100, sa, "test scratch") == 0 && s.get() && s.capacity() == 100);
        const std::vector<Call>& L = hipstub::log();
        CHECK(L.size() == t0 + 4 && L[t0].fn == "hipEventCreate");
        const void* ev = L[t0].a;
        CHECK((L[t0 + 1] == Call{"hipStreamWaitEvent", ev, sa}) && (L[t0 + 2] == Call{"hipEventSynchronize", ev, nullptr}) &&
              (L[t0 + 3] == Call{"hipMalloc", s.get(), nullptr}));
        CHECK(s.release(sa) == 0 && (L.back() == Call{"hipEventRecord", ev, sa}));
        // within capacity, on another stream: the wait alone
        void* p = s.get();
        size_t at = L.size();
        CHECK(s.acquire(64, sb, "test scratch") == 0 && s.get() == p && s.capacity() == 100);
        CHECK(L.size() == at + 1 && (L[at] == Call{"hipStreamWaitEvent", ev, sb}));
        CHECK(s.release(sb) == 0 && (L.back() == Call{"hipEventRecord", ev, sb}));
        CHECK(s.acquire(100, sa, "test scratch") == 0 && L.size() == at + 3);  // (exactly the capacity: no growth)
        // a growth: wait, host synchronise, free, allocate -- in that order
        at = L.size();
        CHECK(s.acquire(101, sb, "test scratch") == 0 && s.capacity() == 101);
        CHECK(L.size() == at + 4 && (L[at] == Call{"hipStreamWaitEvent", ev, sb}) &&
              (L[at + 1] == Call{"hipEventSynchronize", ev, nullptr}) && (L[at + 2] == Call{"hipFree", p, nullptr}) &&
              (L[at + 3] == Call{"hipMalloc", s.get(), nullptr}));
        // a failed growth: empty, FB_ERR_NOMEM and the text; the next acquire succeeds
        hipstub::fail_in() = 1;
        CHECK(s.acquire(500, sa, "test scratch") == kDevmemNoMem && s.get() == nullptr && s.capacity() == 0);
        CHECK(std::string(g_err) == "test scratch (500 bytes)");
        CHECK(hipstub::live().size() == 1);  // (the event)
        CHECK(s.acquire(50, sa, "test scratch") == 0 && s.get() && s.capacity() == 50);
        CHECK(count("hipEventCreate", t0) == 1 && count("hipEventDestroy", t0) == 0);
    }
    CHECK(count("hipEventCreate", t0) == 1 && count("hipEventDestroy", t0) == 1);
    CHECK(count("hipMalloc", t0) == 3 && count("hipFree", t0) == 3 && nothing_live());
}

static void test_event_stream() {
    const size_t t0 = hipstub::log().size();
    {
        DevEvent e;
        DevStream s;
        CHECK(!e && !s);
    }
    CHECK(hipstub::log().size() == t0);  // never used: nothing made, nothing destroyed
    {
        DevEvent e;
        DevStream s;
        CHECK(e.create() == hipSuccess && e.create() == hipSuccess && s.create() == hipSuccess && s.create() == hipSuccess);
        hipEvent_t raw = e;
        DevEvent f(std::move(e));
        CHECK(static_cast<hipEvent_t>(f) == raw && !e);
        DevStream t;
        t = std::move(s);
        CHECK(t && !s);
    }
    CHECK(count("hipEventCreate", t0) == 1 && count("hipEventDestroy", t0) == 1);
    CHECK(count("hipStreamCreate", t0) == 1 && count("hipStreamDestroy", t0) == 1 && nothing_live());
}

int main() {
    test_devbuf();
    test_group();
    test_scratch();
    test_event_stream();
    printf("devmem ok: %zu runtime calls\n", hipstub::log().size());
    hipstub::log().clear();
    return 0;
}
