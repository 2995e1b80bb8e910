/* hip_double.cpp — a HIP runtime made of host memory (see hip_double.h; TEST INFRASTRUCTURE, linked into the sanitizer test
 * programs only).  Every entry point the host-side translation units of the library call is defined here with the runtime's own
 * signature, so that a test program links without libamdhip64 supplying any of them (tests/test_host_double_cpu.py checks the
 * objects' undefined symbols against this file's definitions).
 *
 *   memory   hipMalloc / hipHostMalloc are malloc: ASan sees every byte a copy or a stand-in launcher touches.  A copy checks that
 *            its device side lies inside a live device allocation (of the stream's device) and that its host side does not.
 *   streams  an in-order queue and a worker thread each.  Copies, memsets, event records, event waits and the stand-in
 *            launchers' work are queue entries, so hipEventQuery really answers hipErrorNotReady, work behind a
 *            hipStreamWaitEvent really starts after the event, and a missing wait is a data race TSan can see.
 *   failures the test plans them (hip_double.h): the k-th call overall or of one entry point returns an error code.  These are
 *            return codes of a stand-in in a process that never opens a GPU.
 */
#include "hip_double.h"

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <thread>
#include <vector>

namespace {

enum { K_DEVICE = 0, K_PINNED = 1, K_REGISTERED = 2 };
struct alloc_t { size_t size; int kind; int dev; };

struct event_t {
    std::mutex m;
    std::condition_variable cv;
    uint64_t recorded = 0, completed = 0;
    std::chrono::steady_clock::time_point when{};
};

struct stream_t {
    int dev = 0, ordinal = 0;
    std::mutex m;
    std::condition_variable cv;
    std::deque<std::function<void()>> q;
    bool stop = false;
    std::thread th;
};

struct plan_t { uint64_t k = 0; hipError_t err = hipSuccess; };

struct state_t {
    std::mutex mu;                                    /* allocations, handles, counters, plans */
    int n_devices = 1;
    std::map<uintptr_t, alloc_t> allocs;
    std::map<void *, std::shared_ptr<event_t>> events;
    std::map<void *, std::shared_ptr<stream_t>> streams;
    int next_ordinal = 0;
    std::map<std::string, uint64_t> count;
    std::map<std::string, plan_t> named;
    plan_t overall;
    uint64_t n_overall = 0;
    const char *fired = nullptr;
    std::mutex stall_mu;
    std::condition_variable stall_cv;
    std::set<int> stalled;
    void (*d2h_hook)(const void *, size_t) = nullptr;
};
state_t &S()
{
    static state_t *s = new state_t();                /* never destroyed: workers may outlive main()'s statics */
    return *s;
}
thread_local int t_dev = 0;
thread_local hipError_t t_last = hipSuccess;

/* the live allocation that holds [p, p + len) (mu held) */
const alloc_t *holder(const void *p, size_t len, uintptr_t *base = nullptr)
{
    state_t &s = S();
    const uintptr_t a = (uintptr_t)p;
    auto it = s.allocs.upper_bound(a);
    if (it == s.allocs.begin()) return nullptr;
    --it;
    if (a < it->first || a + len > it->first + it->second.size) return nullptr;
    if (base) *base = it->first;
    return &it->second;
}
/* does [p, p + len) touch a device allocation at all? (mu held) */
bool touches_device(const void *p, size_t len)
{
    state_t &s = S();
    const uintptr_t a = (uintptr_t)p;
    for (auto &kv : s.allocs)
        if (kv.second.kind == K_DEVICE && a < kv.first + kv.second.size && kv.first < a + len) return true;
    return false;
}

hipError_t gate_impl(const char *name, bool is_alloc, bool countable = true)
{
    state_t &s = S();
    std::lock_guard<std::mutex> lk(s.mu);
    const uint64_t c = ++s.count[name];
    hipError_t e = hipSuccess;
    if (countable) {
        ++s.n_overall;
        if (s.overall.k && s.n_overall == s.overall.k) e = s.overall.err != hipSuccess ? s.overall.err : (is_alloc ? hipErrorOutOfMemory : hipErrorUnknown);
    }
    auto it = s.named.find(name);
    if (e == hipSuccess && it != s.named.end() && it->second.k == c) e = it->second.err != hipSuccess ? it->second.err : (is_alloc ? hipErrorOutOfMemory : hipErrorUnknown);
    if (e != hipSuccess) { s.fired = name; t_last = e; }
    return e;
}

std::shared_ptr<stream_t> stream_of(hipStream_t h)
{
    if (!h) return nullptr;
    state_t &s = S();
    std::lock_guard<std::mutex> lk(s.mu);
    auto it = s.streams.find((void *)h);
    if (it == s.streams.end()) hipdbl::die("hip_double: operation on a stream that is not alive (%p)", (void *)h);
    return it->second;
}
std::shared_ptr<event_t> event_of(hipEvent_t h)
{
    state_t &s = S();
    std::lock_guard<std::mutex> lk(s.mu);
    auto it = s.events.find((void *)h);
    if (it == s.events.end()) hipdbl::die("hip_double: operation on an event that is not alive (%p)", (void *)h);
    return it->second;
}

void worker(std::shared_ptr<stream_t> st)
{
    state_t &s = S();
    for (;;) {
        std::function<void()> fn;
        {
            std::unique_lock<std::mutex> lk(st->m);
            st->cv.wait(lk, [&]() { return st->stop || !st->q.empty(); });
            if (st->q.empty()) return;
            fn = std::move(st->q.front());
            st->q.pop_front();
        }
        {
            std::unique_lock<std::mutex> lk(s.stall_mu);
            s.stall_cv.wait(lk, [&]() { return !s.stalled.count(st->ordinal); });
        }
        fn();
    }
}

void push(const std::shared_ptr<stream_t> &st, std::function<void()> fn)
{
    if (!st) { fn(); return; }
    {
        std::lock_guard<std::mutex> lk(st->m);
        if (st->stop) hipdbl::die("hip_double: work queued on a destroyed stream");
        st->q.push_back(std::move(fn));
    }
    st->cv.notify_one();
}

void drain(const std::shared_ptr<stream_t> &st)
{
    if (!st) return;
    struct flag_t { std::mutex m; std::condition_variable cv; bool done = false; };
    auto f = std::make_shared<flag_t>();
    push(st, [f]() { { std::lock_guard<std::mutex> lk(f->m); f->done = true; } f->cv.notify_all(); });
    std::unique_lock<std::mutex> lk(f->m);
    f->cv.wait(lk, [&]() { return f->done; });
}

hipError_t new_stream(hipStream_t *out)
{
    state_t &s = S();
    auto st = std::make_shared<stream_t>();
    st->dev = t_dev;
    {
        std::lock_guard<std::mutex> lk(s.mu);
        st->ordinal = s.next_ordinal++;
        s.streams[(void *)st.get()] = st;
    }
    st->th = std::thread(worker, st);
    *out = (hipStream_t)st.get();
    return hipSuccess;
}

/* a copy's two ranges against the allocation table; dev: the stream's device (-1: not known) */
void check_copy(const void *dst, const void *src, size_t n, hipMemcpyKind kind, int dev, const char *who)
{
    if (!n) return;
    state_t &s = S();
    std::lock_guard<std::mutex> lk(s.mu);
    const bool to_dev = kind == hipMemcpyHostToDevice || kind == hipMemcpyDeviceToDevice;
    const bool from_dev = kind == hipMemcpyDeviceToHost || kind == hipMemcpyDeviceToDevice;
    if (kind != hipMemcpyHostToDevice && kind != hipMemcpyDeviceToHost && kind != hipMemcpyDeviceToDevice)
        hipdbl::die("hip_double: %s with a copy kind the library is not known to use (%d)", who, (int)kind);
    const alloc_t *d = holder(dst, n), *r = holder(src, n);
    if (to_dev && !(d && d->kind == K_DEVICE)) hipdbl::die("hip_double: %s: destination [%p, +%zu) is not inside a live device allocation", who, dst, n);
    if (from_dev && !(r && r->kind == K_DEVICE)) hipdbl::die("hip_double: %s: source [%p, +%zu) is not inside a live device allocation", who, src, n);
    if (!to_dev && touches_device(dst, n)) hipdbl::die("hip_double: %s: host destination [%p, +%zu) overlaps device memory", who, dst, n);
    if (!from_dev && touches_device(src, n)) hipdbl::die("hip_double: %s: host source [%p, +%zu) overlaps device memory", who, src, n);
    if (dev >= 0 && to_dev && d->dev != dev) hipdbl::die("hip_double: %s: destination lives on device %d, the stream on device %d", who, d->dev, dev);
    if (dev >= 0 && from_dev && r->dev != dev) hipdbl::die("hip_double: %s: source lives on device %d, the stream on device %d", who, r->dev, dev);
}

}  // namespace

/* ================================================================ control interface */
namespace hipdbl {

void die(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
    fflush(stderr);
    abort();
}

void release_streams()
{
    state_t &s = S();
    { std::lock_guard<std::mutex> lk(s.stall_mu); s.stalled.clear(); }
    s.stall_cv.notify_all();
}

void stall_stream(int k)
{
    state_t &s = S();
    std::lock_guard<std::mutex> lk(s.stall_mu);
    s.stalled.insert(k);
}

void reset(int n_devices)
{
    state_t &s = S();
    release_streams();
    std::vector<std::shared_ptr<stream_t>> live;
    {
        std::lock_guard<std::mutex> lk(s.mu);
        for (auto &kv : s.streams) live.push_back(kv.second);
    }
    for (auto &st : live) {
        { std::lock_guard<std::mutex> lk(st->m); st->stop = true; }
        st->cv.notify_all();
        if (st->th.joinable()) st->th.join();
    }
    std::lock_guard<std::mutex> lk(s.mu);
    s.streams.clear();
    s.events.clear();
    for (auto &kv : s.allocs)
        if (kv.second.kind != K_REGISTERED) free((void *)kv.first);
    s.allocs.clear();
    s.count.clear();
    s.named.clear();
    s.overall = plan_t();
    s.n_overall = 0;
    s.fired = nullptr;
    s.next_ordinal = 0;
    s.n_devices = n_devices;
    t_dev = 0;
    t_last = hipSuccess;
}

void enqueue(hipStream_t h, std::function<void()> fn) { push(stream_of(h), std::move(fn)); }
hipError_t gate(const char *name, bool is_alloc) { return gate_impl(name, is_alloc); }
int device_of_stream(hipStream_t h) { auto st = stream_of(h); return st ? st->dev : -1; }
int device_of_ptr(const void *p, size_t len)
{
    state_t &s = S();
    std::lock_guard<std::mutex> lk(s.mu);
    const alloc_t *a = holder(p, len ? len : 1);
    return a && a->kind == K_DEVICE ? a->dev : -1;
}
void set_d2h_hook(void (*fn)(const void *, size_t)) { std::lock_guard<std::mutex> lk(S().mu); S().d2h_hook = fn; }

uint64_t calls(const char *name)
{
    state_t &s = S();
    std::lock_guard<std::mutex> lk(s.mu);
    auto it = s.count.find(name);
    return it == s.count.end() ? 0 : it->second;
}
uint64_t overall_calls() { std::lock_guard<std::mutex> lk(S().mu); return S().n_overall; }
void reset_counters()
{
    state_t &s = S();
    std::lock_guard<std::mutex> lk(s.mu);
    s.count.clear();
    s.n_overall = 0;
    s.fired = nullptr;
}
void fail_overall(uint64_t k, hipError_t err) { std::lock_guard<std::mutex> lk(S().mu); S().overall.k = k; S().overall.err = err; }
void fail_named(const char *name, uint64_t k, hipError_t err) { std::lock_guard<std::mutex> lk(S().mu); S().named[name] = plan_t{k, err}; }
void clear_failures() { std::lock_guard<std::mutex> lk(S().mu); S().named.clear(); S().overall = plan_t(); }
const char *fired() { std::lock_guard<std::mutex> lk(S().mu); return S().fired; }
size_t live_objects()
{
    state_t &s = S();
    std::lock_guard<std::mutex> lk(s.mu);
    return s.allocs.size() + s.streams.size() + s.events.size();
}

}  // namespace hipdbl

/* ================================================================ the runtime's entry points */
#define GATE(name, is_alloc)                                       \
    do {                                                           \
        const hipError_t g_ = gate_impl(name, is_alloc);           \
        if (g_ != hipSuccess) return g_;                           \
    } while (0)

extern "C" {

hipError_t hipGetDeviceCount(int *n)
{
    GATE("hipGetDeviceCount", false);
    std::lock_guard<std::mutex> lk(S().mu);
    *n = S().n_devices;
    return hipSuccess;
}

hipError_t hipSetDevice(int d)
{
    GATE("hipSetDevice", false);
    { std::lock_guard<std::mutex> lk(S().mu); if (d < 0 || d >= S().n_devices) return t_last = hipErrorInvalidDevice; }
    t_dev = d;
    return hipSuccess;
}

hipError_t hipGetDeviceProperties(hipDeviceProp_t *pr, int d)
{
    GATE("hipGetDeviceProperties", false);
    { std::lock_guard<std::mutex> lk(S().mu); if (d < 0 || d >= S().n_devices) return t_last = hipErrorInvalidDevice; }
    memset(pr, 0, sizeof(*pr));
    snprintf(pr->name, sizeof(pr->name), "host-memory stand-in %d", d);
    snprintf(pr->gcnArchName, sizeof(pr->gcnArchName), "gfx950");
    pr->multiProcessorCount = 256;
    pr->warpSize = 64;
    return hipSuccess;
}

hipError_t hipDeviceGetPCIBusId(char *bdf, int len, int d)
{
    GATE("hipDeviceGetPCIBusId", false);
    { std::lock_guard<std::mutex> lk(S().mu); if (d < 0 || d >= S().n_devices) return t_last = hipErrorInvalidDevice; }
    snprintf(bdf, (size_t)len, "0000:%02X:00.0", 0xA1 + 0x0B * d);      /* made up; upper case, as the runtime answers */
    return hipSuccess;
}

hipError_t hipDeviceGetStreamPriorityRange(int *least, int *greatest)
{
    GATE("hipDeviceGetStreamPriorityRange", false);
    if (least) *least = 1;
    if (greatest) *greatest = -1;
    return hipSuccess;
}

hipError_t hipGetLastError(void)
{
    (void)gate_impl("hipGetLastError", false, false);
    const hipError_t e = t_last;
    t_last = hipSuccess;
    return e;
}

const char *hipGetErrorString(hipError_t e)
{
    switch (e) {
    case hipSuccess: return "no error";
    case hipErrorOutOfMemory: return "out of memory";
    case hipErrorNotReady: return "device not ready";
    case hipErrorInvalidDevice: return "invalid device ordinal";
    case hipErrorInvalidValue: return "invalid argument";
    case hipErrorUnknown: return "unknown error";
    default: return "some error";
    }
}

/* ---- memory ---- */
static hipError_t alloc_common(void **p, size_t bytes, int kind)
{
    if (!p) return t_last = hipErrorInvalidValue;
    *p = nullptr;
    if (!bytes) return hipSuccess;
    void *m = malloc(bytes);
    if (!m) return t_last = hipErrorOutOfMemory;
    std::lock_guard<std::mutex> lk(S().mu);
    S().allocs[(uintptr_t)m] = alloc_t{bytes, kind, t_dev};
    *p = m;
    return hipSuccess;
}
static hipError_t free_common(void *p, int kind, const char *who)
{
    if (!p) return hipSuccess;
    {
        std::lock_guard<std::mutex> lk(S().mu);
        auto it = S().allocs.find((uintptr_t)p);
        if (it == S().allocs.end() || it->second.kind != kind) hipdbl::die("hip_double: %s(%p): not a live allocation of that kind (double free?)", who, p);
        S().allocs.erase(it);
    }
    if (kind != K_REGISTERED) free(p);
    return hipSuccess;
}

hipError_t hipMalloc(void **p, size_t bytes) { GATE("hipMalloc", true); return alloc_common(p, bytes, K_DEVICE); }
hipError_t hipFree(void *p)
{
    const hipError_t g = gate_impl("hipFree", false);
    (void)free_common(p, K_DEVICE, "hipFree");
    return g;
}
hipError_t hipHostMalloc(void **p, size_t bytes, unsigned int) { GATE("hipHostMalloc", true); return alloc_common(p, bytes, K_PINNED); }
hipError_t hipHostFree(void *p)
{
    const hipError_t g = gate_impl("hipHostFree", false);
    (void)free_common(p, K_PINNED, "hipHostFree");
    return g;
}
hipError_t hipHostRegister(void *p, size_t bytes, unsigned int)
{
    GATE("hipHostRegister", false);
    if (!p || !bytes) return t_last = hipErrorInvalidValue;
    std::lock_guard<std::mutex> lk(S().mu);
    if (S().allocs.count((uintptr_t)p)) return t_last = hipErrorHostMemoryAlreadyRegistered;
    S().allocs[(uintptr_t)p] = alloc_t{bytes, K_REGISTERED, -1};
    return hipSuccess;
}
hipError_t hipHostUnregister(void *p)
{
    const hipError_t g = gate_impl("hipHostUnregister", false);
    (void)free_common(p, K_REGISTERED, "hipHostUnregister");
    return g;
}

hipError_t hipMemcpy(void *dst, const void *src, size_t n, hipMemcpyKind kind)
{
    GATE("hipMemcpy", false);
    check_copy(dst, src, n, kind, -1, "hipMemcpy");
    if (kind == hipMemcpyDeviceToHost) {
        void (*hook)(const void *, size_t);
        { std::lock_guard<std::mutex> lk(S().mu); hook = S().d2h_hook; }
        if (hook) hook(src, n);
    }
    if (n) memcpy(dst, src, n);
    return hipSuccess;
}

hipError_t hipMemcpyAsync(void *dst, const void *src, size_t n, hipMemcpyKind kind, hipStream_t h)
{
    GATE("hipMemcpyAsync", false);
    auto st = stream_of(h);
    const int dev = st ? st->dev : -1;
    check_copy(dst, src, n, kind, dev, "hipMemcpyAsync");
    push(st, [=]() {
        check_copy(dst, src, n, kind, dev, "hipMemcpyAsync (when the copy runs)");       /* the buffers must still be alive */
        if (kind == hipMemcpyDeviceToHost) {
            void (*hook)(const void *, size_t);
            { std::lock_guard<std::mutex> lk(S().mu); hook = S().d2h_hook; }
            if (hook) hook(src, n);
        }
        if (n) memcpy(dst, src, n);
    });
    return hipSuccess;
}

static void check_device_range(const void *p, size_t n, int dev, const char *who)
{
    if (!n) return;
    std::lock_guard<std::mutex> lk(S().mu);
    const alloc_t *a = holder(p, n);
    if (!a || a->kind != K_DEVICE) hipdbl::die("hip_double: %s: [%p, +%zu) is not inside a live device allocation", who, p, n);
    if (dev >= 0 && a->dev != dev) hipdbl::die("hip_double: %s: memory of device %d on a stream of device %d", who, a->dev, dev);
}

hipError_t hipMemset(void *p, int v, size_t n)
{
    GATE("hipMemset", false);
    check_device_range(p, n, -1, "hipMemset");
    if (n) memset(p, v, n);
    return hipSuccess;
}

hipError_t hipMemsetAsync(void *p, int v, size_t n, hipStream_t h)
{
    GATE("hipMemsetAsync", false);
    auto st = stream_of(h);
    const int dev = st ? st->dev : -1;
    check_device_range(p, n, dev, "hipMemsetAsync");
    push(st, [=]() {
        check_device_range(p, n, dev, "hipMemsetAsync (when it runs)");
        if (n) memset(p, v, n);
    });
    return hipSuccess;
}

/* ---- streams ---- */
hipError_t hipStreamCreateWithFlags(hipStream_t *out, unsigned int) { GATE("hipStreamCreateWithFlags", false); return new_stream(out); }
hipError_t hipStreamCreateWithPriority(hipStream_t *out, unsigned int, int) { GATE("hipStreamCreateWithPriority", false); return new_stream(out); }
hipError_t hipStreamCreate(hipStream_t *out) { GATE("hipStreamCreate", false); return new_stream(out); }

hipError_t hipStreamDestroy(hipStream_t h)
{
    const hipError_t g = gate_impl("hipStreamDestroy", false);
    std::shared_ptr<stream_t> st;
    {
        std::lock_guard<std::mutex> lk(S().mu);
        auto it = S().streams.find((void *)h);
        if (it == S().streams.end()) hipdbl::die("hip_double: hipStreamDestroy(%p): not a live stream (destroyed twice?)", (void *)h);
        st = it->second;
        S().streams.erase(it);
    }
    { std::lock_guard<std::mutex> lk(st->m); st->stop = true; }       /* (the worker finishes what is queued first) */
    st->cv.notify_all();
    st->th.join();
    return g;
}

hipError_t hipStreamSynchronize(hipStream_t h)
{
    GATE("hipStreamSynchronize", false);
    drain(stream_of(h));
    return hipSuccess;
}

hipError_t hipStreamWaitEvent(hipStream_t h, hipEvent_t eh, unsigned int)
{
    GATE("hipStreamWaitEvent", false);
    auto st = stream_of(h);
    auto ev = event_of(eh);
    uint64_t target;
    { std::lock_guard<std::mutex> lk(ev->m); target = ev->recorded; }      /* the record the event holds NOW, as the runtime captures it */
    push(st, [ev, target]() {
        std::unique_lock<std::mutex> lk(ev->m);
        ev->cv.wait(lk, [&]() { return ev->completed >= target; });
    });
    return hipSuccess;
}

/* ---- events ---- */
static hipError_t new_event(hipEvent_t *out)
{
    auto ev = std::make_shared<event_t>();
    std::lock_guard<std::mutex> lk(S().mu);
    S().events[(void *)ev.get()] = ev;
    *out = (hipEvent_t)ev.get();
    return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t *out) { GATE("hipEventCreate", false); return new_event(out); }
hipError_t hipEventCreateWithFlags(hipEvent_t *out, unsigned int) { GATE("hipEventCreateWithFlags", false); return new_event(out); }

hipError_t hipEventDestroy(hipEvent_t h)
{
    const hipError_t g = gate_impl("hipEventDestroy", false);
    std::lock_guard<std::mutex> lk(S().mu);
    if (!S().events.erase((void *)h)) hipdbl::die("hip_double: hipEventDestroy(%p): not a live event (destroyed twice?)", (void *)h);
    return g;                                           /* (queued records and waits keep the object alive) */
}

hipError_t hipEventRecord(hipEvent_t eh, hipStream_t h)
{
    GATE("hipEventRecord", false);
    auto st = stream_of(h);
    auto ev = event_of(eh);
    uint64_t target;
    { std::lock_guard<std::mutex> lk(ev->m); target = ++ev->recorded; }
    push(st, [ev, target]() {
        { std::lock_guard<std::mutex> lk(ev->m); if (ev->completed < target) ev->completed = target; ev->when = std::chrono::steady_clock::now(); }
        ev->cv.notify_all();
    });
    return hipSuccess;
}

hipError_t hipEventQuery(hipEvent_t eh)
{
    auto ev = event_of(eh);
    bool ready;
    { std::lock_guard<std::mutex> lk(ev->m); ready = ev->completed >= ev->recorded; }
    if (!ready) { (void)gate_impl("hipEventQuery", false, false); return hipErrorNotReady; }     /* (not an error: t_last stays) */
    GATE("hipEventQuery", false);
    return hipSuccess;
}

hipError_t hipEventSynchronize(hipEvent_t eh)
{
    GATE("hipEventSynchronize", false);
    auto ev = event_of(eh);
    std::unique_lock<std::mutex> lk(ev->m);
    const uint64_t target = ev->recorded;
    ev->cv.wait(lk, [&]() { return ev->completed >= target; });
    return hipSuccess;
}

hipError_t hipEventElapsedTime(float *ms, hipEvent_t a, hipEvent_t b)
{
    GATE("hipEventElapsedTime", false);
    auto ea = event_of(a), eb = event_of(b);
    std::chrono::steady_clock::time_point ta, tb;
    { std::lock_guard<std::mutex> lk(ea->m); if (!ea->recorded) return t_last = hipErrorInvalidHandle; if (ea->completed < ea->recorded) return hipErrorNotReady; ta = ea->when; }
    { std::lock_guard<std::mutex> lk(eb->m); if (!eb->recorded) return t_last = hipErrorInvalidHandle; if (eb->completed < eb->recorded) return hipErrorNotReady; tb = eb->when; }
    *ms = std::chrono::duration<float, std::milli>(tb - ta).count();
    return hipSuccess;
}

}  // extern "C"
