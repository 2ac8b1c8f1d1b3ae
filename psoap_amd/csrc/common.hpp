// common.hpp -- shared types and constants for the gfx950 GP-likelihood kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include <utility>
#include "tile_consts.hpp"

namespace psoap {

typedef double d4 __attribute__((ext_vector_type(4)));
typedef double d2 __attribute__((ext_vector_type(2)));

constexpr int LDS_LD = 144;   // LDS row stride (doubles): 128 + 16 keeps ds_read_b64 fragment
                              // reads of two consecutive k-rows on disjoint bank halves
constexpr int GEMM_THREADS = 256;
constexpr size_t GEMM_LDS_BYTES = (size_t)2 /*operands*/ * 2 /*buffers*/ * KB * LDS_LD * sizeof(double);

// What the factorisation of ONE diagonal block contributes to lnprob.  A matrix owns ACC_ROWS of these records, one per
// block row (record q is written by the task that factors diagonal block q and by nobody else); whoever reports the
// result adds them up in the order q = 0, 1, ..., P-1 (acc_total).
// Rounds 1-5 kept ONE record per matrix that every diagonal task read, added to and wrote back -- a read-modify-write
// chain whose only ordering was the dependency of diagonal task q+1 on diagonal task q.  The second level of following
// (scheme 2, round 3) removed that dependency: task q+1 follows the strip solve that follows the steps of task q and
// never waits for anything task q publishes AFTER its accumulator update, so nothing ordered the two updates but time
// (task q+1 still has a block to factor, ~40 us) -- and with the records of four matrices in one 128-byte line a workgroup
// of another XCD could read the line for a neighbouring matrix (the result report of a stream lane), leave a snapshot of
// it in that XCD's L2, and a diagonal task that XCD ran next (a stolen one: its own lane had just finished) started from
// that snapshot: exactly one block row's contribution missing from lnprob -- the wrong value (2-3 % low) once in 20,000
// (N = 8192) ... 80,000 (N = 4096) matrices through a resident launch with the following scheme that round 5 found and
// fenced (profiles/r5_stream_scheme2.txt; every large mismatch there equals -0.5 (z_q^T z_q + 2 sum log U_ii) of ONE block
// q in {1, 29, 30, 31} to the last digit: profiles/r6_acc_forensics.txt).  No chain, no shared line: nothing to order.
struct MatAcc {
    double logdet_half;  // sum_i log U_ii over the block's 128 pivots   (logdet K = 2 * the sum over blocks)
    double quad;         // z_q^T z_q, z = U^-T r
    double info;         // != 0  ->  a pivot was <= 0 or NaN (not positive definite)
    double pad;
};
constexpr int ACC_ROWS = 256;      // records per matrix (block rows are 8-bit indices): 8 KiB, a whole number of 128-byte lines
static_assert(sizeof(MatAcc) == 32 && (ACC_ROWS * sizeof(MatAcc)) % 128 == 0, "a matrix's records share no cache line with another's");

// the record of diagonal block k0 / NB, written through (thread 0 of the factoring workgroup, or of a staged kernel)
__device__ __forceinline__ void acc_store(MatAcc* acc, int q, double logdet_half, double quad, bool bad)
{
    __hip_atomic_store(&acc[q].logdet_half, logdet_half, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&acc[q].quad, quad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&acc[q].info, bad ? 1.0 : 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Reading a word that other workgroups write (a progress flag, a ticket counter): the value the MEMORY holds now.
// Every poll of the persistent kernels goes through here.  Rounds 1-5 wrote their polls as `__hip_atomic_fetch_add(p, 0)`
// on the understanding that a read-modify-write executes at the memory side -- and hipcc turned every one of them into a
// load: LLVM folds an atomic read-modify-write whose operand is the operation's identity (add 0, or 0) and whose ordering
// is relaxed into an ATOMIC LOAD (`flat_load_dword ... sc1`, 2868 of them in the round-5 binary), which the XCD's L2 may
// serve.  In rmw_read the zero passes through an opaque statement, the fold cannot happen and the read is the returning
// atomic add (round 6's A/B: the polls do not need it -- `sc1` loads are coherent -- and are 1.2 % slower with it).
template <class T>
__device__ __forceinline__ T rmw_read(T* p)      // always the returning atomic add (executed at the memory side, past every L2)
{
    T z = 0;
    asm volatile("" : "+v"(z));
    return __hip_atomic_fetch_add(p, z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <class T>
__device__ __forceinline__ T poll_word(T* p)
{
    return __hip_atomic_fetch_add(p, (T)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// row-major upper-triangle tile index t in [0, P(P+1)/2)  ->  (ti, tj), tj >= ti
__device__ inline void decode_upper(int t, int P, int& ti, int& tj)
{
    // row ti starts at offset ti*P - ti*(ti-1)/2
    double twoP1 = 2.0 * P + 1.0;
    int r = (int)((twoP1 - sqrt(twoP1 * twoP1 - 8.0 * (double)t)) * 0.5);
    if (r < 0) r = 0;
    if (r > P - 1) r = P - 1;
    while (r > 0 && r * P - r * (r - 1) / 2 > t) --r;
    while ((r + 1) * P - (r + 1) * r / 2 <= t) ++r;
    ti = r;
    tj = r + (t - (r * P - r * (r - 1) / 2));
}

// The sum of one value per thread of a 256-thread workgroup through red[256] in LDS: store, barrier, then eight halvings with a
// barrier behind each -- a fixed order of additions.  Every thread returns the sum; a caller that uses `red` again puts a
// barrier in between.
__device__ __forceinline__ double block_sum_256(double* red, double v)
{
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int w = 128; w >= 1; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    return red[0];
}

// ---- host ----------------------------------------------------------------------------------
// The owners.  A field that holds a device resource is one of these: it is released where the field goes out of scope, on
// every return path, and no destroy function names it.  All are move-only and convert to the raw handle.
//
// Grow: a grow-only device (or pinned host) buffer.  need() allocates only when a call outgrows it (a workspace reused call
// after call allocates nothing).  `flags`: hipHostMalloc's, for the pinned form.
template <class T, bool HOST = false>
struct Grow {
    static constexpr bool pinned = HOST;
    T* p = nullptr;
    size_t cap = 0;
    unsigned int flags = hipHostMallocDefault;
    Grow() = default;
    explicit Grow(unsigned int host_flags) : flags(host_flags) {}
    Grow(Grow&& o) noexcept : p(o.p), cap(o.cap), flags(o.flags) { o.p = nullptr, o.cap = 0; }
    Grow& operator=(Grow&& o) noexcept      // (a swap: what this one held goes with `o`)
    {
        std::swap(p, o.p), std::swap(cap, o.cap), std::swap(flags, o.flags);
        return *this;
    }
    ~Grow() { release(); }
    void release()
    {
        if (p) (void)(HOST ? hipHostFree(p) : hipFree(p));
        p = nullptr;
        cap = 0;
    }
    hipError_t need(size_t count)
    {
        if (count <= cap && p) return hipSuccess;
        release();
        const hipError_t e = HOST ? hipHostMalloc(reinterpret_cast<void**>(&p), sizeof(T) * count, flags)
                                  : hipMalloc(reinterpret_cast<void**>(&p), sizeof(T) * count);
        if (e == hipSuccess) cap = count;
        else p = nullptr;
        return e;
    }
    operator T*() const { return p; }
    T* operator->() const { return p; }
};

// a stream of its own (hipStreamNonBlocking)
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(Stream&& o) noexcept : s(o.s) { o.s = nullptr; }
    Stream& operator=(Stream&& o) noexcept { return std::swap(s, o.s), *this; }
    ~Stream() { release(); }
    void release() { if (s) (void)hipStreamDestroy(s); s = nullptr; }
    hipError_t create() { release(); return hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
    operator hipStream_t() const { return s; }
};

// an event: an ordering mark (hipEventDisableTiming) unless it is created to be timed (hipEventDefault)
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; }
    Event& operator=(Event&& o) noexcept { return std::swap(e, o.e), *this; }
    ~Event() { release(); }
    void release() { if (e) (void)hipEventDestroy(e); e = nullptr; }
    hipError_t create(unsigned int flags = hipEventDisableTiming) { release(); return hipEventCreateWithFlags(&e, flags); }
    operator hipEvent_t() const { return e; }
};

// A runtime component count (1 .. 3) as a compile-time one: f(std::integral_constant<int, C>()), for the kernels that are
// templates over it.
template <class F>
inline void with_components(int c, F&& f)
{
    if (c == 1) f(std::integral_constant<int, 1>());
    else if (c == 2) f(std::integral_constant<int, 2>());
    else f(std::integral_constant<int, 3>());
}

}  // namespace psoap
