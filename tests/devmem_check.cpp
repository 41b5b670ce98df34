// devmem_check.cpp -- stand-alone checks of rgbd-slam_amd/csrc/devmem.h, built and run by tests/test_devmem.py
// (mode "fail": needs no device) and tests/test_gpu_devmem.py (mode "ok": needs one).
#include "devmem.h"

#include <dlfcn.h>

#include <cstdio>
#include <cstring>
#include <utility>

using namespace rgbd;

static int g_bad = 0, g_destroys = 0, g_null_destroys = 0;

#define CHECK(x)                                                   \
    do {                                                           \
        if (!(x)) {                                                \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); \
            g_bad++;                                               \
        }                                                          \
    } while (0)

// counts the calls Event's destructor makes, then forwards to the runtime
extern "C" hipError_t hipEventDestroy(hipEvent_t e)
{
    g_destroys++;
    if (!e) g_null_destroys++;
    using Fn = hipError_t (*)(hipEvent_t);
    static const Fn next = reinterpret_cast<Fn>(dlsym(RTLD_NEXT, "hipEventDestroy"));
    return next ? next(e) : hipErrorUnknown;
}

// a request no machine can serve: without a device every allocation fails, with one this size does
constexpr size_t kHuge = size_t(1) << 60;

template <typename B>
static void failing_buffer()
{
    B b;
    CHECK(b.get() == nullptr && b.capacity() == 0);
    CHECK(b.reserve(kHuge) != hipSuccess);
    CHECK(b.get() == nullptr && b.capacity() == 0);
    CHECK(b.reserve(kHuge) != hipSuccess);   // the allocator was asked again: a skipped reserve returns hipSuccess
    CHECK(b.get() == nullptr && b.capacity() == 0);
    CHECK(b.alloc(kHuge) != hipSuccess);
    CHECK(b.get() == nullptr && b.capacity() == 0);
    CHECK(b.reserve(0) == hipSuccess && b.get() == nullptr);   // nothing asked, nothing allocated
    B empty, from_empty(std::move(empty));
    CHECK(empty.get() == nullptr && empty.capacity() == 0 && from_empty.get() == nullptr && from_empty.capacity() == 0);
    B from_failed;
    from_failed = std::move(b);
    CHECK(b.get() == nullptr && b.capacity() == 0 && from_failed.get() == nullptr && from_failed.capacity() == 0);
    b.release();   // releasing an empty buffer is a no-op
}

static int mode_fail()
{
    failing_buffer<DevBuf<unsigned char>>();
    failing_buffer<PinnedBuf<unsigned char>>();
    failing_buffer<DevBuf<double>>();
    int ndev = 0;
    const bool device = hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0;
    {
        Event e;
        const hipError_t r = e.ensure();
        if (!device) {   // the error is reported, the event stays null and is never destroyed
            CHECK(r != hipSuccess);
            CHECK((hipEvent_t)e == nullptr);
            CHECK(e.ensure() != hipSuccess);
        } else {
            CHECK(r == hipSuccess && (hipEvent_t)e != nullptr);
        }
    }
    CHECK(g_destroys == (device ? 1 : 0));
    { Event never_used; }
    CHECK(g_destroys == (device ? 1 : 0) && g_null_destroys == 0);
    return g_bad;
}

static size_t allocation_bytes(void* p)
{
    hipDeviceptr_t base = nullptr;
    size_t bytes = 0;
    return hipMemGetAddressRange(&base, &bytes, p) == hipSuccess ? bytes : 0;
}

static int mode_ok()
{
    DevBuf<int> d;
    CHECK(d.alloc(0) == hipSuccess && d.get() != nullptr && d.capacity() == 0);
    CHECK(hipMemset(d, 0, 16) == hipSuccess);   // the 16-byte floor
    CHECK(d.reserve(100) == hipSuccess && d.capacity() == 100);
    int* const p100 = d;
    const size_t s100 = allocation_bytes(p100);
    CHECK(d.reserve(150) == hipSuccess && d.capacity() == 200);   // max(n, 2 x capacity)
    int* const p200 = d;
    const size_t s200 = allocation_bytes(p200);
    // reserve releases before it allocates, so the runtime may hand the same address out again: what shows the
    // new allocation is its size, which the first one did not have
    std::printf("reserve(100) -> %p, %zu B; reserve(150) -> %p, %zu B\n", (void*)p100, s100, (void*)p200, s200);
    CHECK(p200 != nullptr && s100 >= 100 * sizeof(int) && s100 < 200 * sizeof(int) && s200 >= 200 * sizeof(int));
    CHECK(hipMemset(d, 0, 200 * sizeof(int)) == hipSuccess);
    CHECK(d.reserve(150) == hipSuccess && d.get() == p200 && d.capacity() == 200);
    DevBuf<int> t;
    CHECK(t.alloc(4) == hipSuccess);
    t = std::move(d);
    CHECK(t.get() == p200 && t.capacity() == 200 && d.get() == nullptr && d.capacity() == 0);
    DevBuf<int> m(std::move(t));
    CHECK(m.get() == p200 && t.get() == nullptr);
    PinnedBuf<int> h;
    CHECK(h.reserve(200) == hipSuccess && h.capacity() == 200);
    std::memset(h, 0, 200 * sizeof(int));
    CHECK(hipMemset(m, 0x5a, 200 * sizeof(int)) == hipSuccess);
    CHECK(hipMemcpy(h, m, 200 * sizeof(int), hipMemcpyDeviceToHost) == hipSuccess);
    bool same = true;
    for (int i = 0; i < 200; i++) same = same && h[i] == 0x5a5a5a5a;
    CHECK(same);
    {
        Event e;
        CHECK((hipEvent_t)e == nullptr);
        CHECK(e.ensure() == hipSuccess && (hipEvent_t)e != nullptr);
        const hipEvent_t first = e;
        CHECK(e.ensure() == hipSuccess && (hipEvent_t)e == first);   // created once
        CHECK(hipEventRecord(e, nullptr) == hipSuccess && hipEventSynchronize(e) == hipSuccess);
    }
    CHECK(g_destroys == 1 && g_null_destroys == 0);
    return g_bad;
}

int main(int argc, char** argv)
{
    const bool ok_mode = argc > 1 && !std::strcmp(argv[1], "ok");
    const int bad = ok_mode ? mode_ok() : mode_fail();
    if (!bad) std::printf("devmem_check %s: all checks passed\n", ok_mode ? "ok" : "fail");
    return bad ? 1 : 0;
}
