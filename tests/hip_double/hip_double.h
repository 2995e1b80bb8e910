/* hip_double.h — control interface of the host-memory HIP stand-in (tests/hip_double/hip_double.cpp).
 *
 * TEST INFRASTRUCTURE.  The double is an object file of the sanitizer test programs: it is never built into
 * libbwasw_mi355.so, never preloaded, and no switch in the product library knows of it.  It defines, with the runtime's own
 * signatures, every HIP entry point the host-side translation units use; "device memory" is malloc'ed host memory, a stream is
 * an in-order queue with a worker thread of its own, an event fires when its stream's worker reaches the record.  It says
 * nothing about the real runtime's behaviour, about kernels, or about timing.
 */
#ifndef BSW_HIP_DOUBLE_H
#define BSW_HIP_DOUBLE_H

#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include <functional>

namespace hipdbl {

/* Forget everything: joins the stream workers, frees whatever is still allocated (a context marked dead leaks its streams and
 * buffers on purpose), clears counters, failures and stalls; n_devices "gfx950" devices from now on. */
void reset(int n_devices);

/* ---- what the stand-in launchers need ---- */
/* work queued on a stream, run by its worker in order (s == nullptr: run at once, on the caller) */
void enqueue(hipStream_t s, std::function<void()> fn);
/* counts one call of the named entry point (a launcher's name) and answers the failure the test planned for it */
hipError_t gate(const char *name, bool is_alloc = false);
int device_of_stream(hipStream_t s);                 /* -1: the null stream */
int device_of_ptr(const void *p, size_t len);        /* device of the live device allocation that holds [p, p + len); -1: none */
/* called on the worker, in front of every device-to-host copy, with the copy's source */
void set_d2h_hook(void (*fn)(const void *src, size_t bytes));
[[noreturn]] void die(const char *fmt, ...) __attribute__((format(printf, 1, 2)));

/* ---- what the test programs steer ---- */
uint64_t calls(const char *name);                    /* calls of one entry point since the last reset / reset_counters */
/* calls of ALL entry points and launchers that could have failed: every call but hipGetErrorString and a hipEventQuery that
 * answers hipErrorNotReady (a poll that found nothing; their number depends on timing) */
uint64_t overall_calls();
void reset_counters();
/* the k-th (1-based) call overall / of the named entry point from now on fails: hipErrorOutOfMemory from an allocation,
 * hipErrorUnknown otherwise (err != hipSuccess: that code).  A failing release (hipFree, hipEventDestroy, ...) still releases:
 * the double must not turn an ignored return code into a leak report. */
void fail_overall(uint64_t k, hipError_t err = hipSuccess);
void fail_named(const char *name, uint64_t k, hipError_t err = hipSuccess);
void clear_failures();
const char *fired();                                 /* the entry point whose planned failure has happened; nullptr: none yet */
/* the worker of the k-th stream created since the last reset (0-based) sleeps in front of its next operation until released */
void stall_stream(int k);
void release_streams();
size_t live_objects();                               /* device and pinned allocations, registrations, streams and events alive */

}  // namespace hipdbl

#endif
