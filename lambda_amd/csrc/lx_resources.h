// lx_resources.h -- the owners of what the handle (lx_internal.h) and lx_taxmap (lx_taxmap_host.cpp) hold of the runtime: device
// blocks, pinned blocks, events, streams.  All move-only; a destructor gives back what it holds.  None remembers a device: whoever
// owns them binds its device, and synchronises its streams, before the first of them goes (lx_handle's destructor).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <type_traits>
#include <utility>

struct lx_handle;

namespace lxi
{

// A block that grows on demand (ensure / ensure_pinned below): where it is and what it holds.
template <hipError_t (*kFree)(void *)>
struct Buf
{
    void * ptr = nullptr;
    size_t cap = 0;
    Buf()      = default;
    Buf(Buf const &) = delete;
    Buf & operator=(Buf const &) = delete;
    Buf(Buf && o) noexcept : ptr(std::exchange(o.ptr, nullptr)), cap(std::exchange(o.cap, 0)) {}
    Buf & operator=(Buf && o) noexcept
    {
        std::swap(ptr, o.ptr);
        std::swap(cap, o.cap);
        return *this;
    }
    ~Buf()
    {
        if (ptr)
            (void)kFree(ptr);
    }
};
using DevBuf = Buf<hipFree>;     // hipMalloc
using Pinned = Buf<hipHostFree>; // hipHostMalloc

// One object of the runtime -- an event, a stream, a block of a fixed size seen as T * -- and the call that gives it back.  Converts
// to the raw type, so the runtime's calls take it as they take that.  Made where it is first needed, through out():
// hipEventCreateWithFlags(ev.out(), hipEventDisableTiming), hipMalloc(block.out(), bytes).
template <class T, auto kRelease>
struct Owner
{
    T raw = nullptr;
    Owner() = default;
    Owner(Owner const &) = delete;
    Owner & operator=(Owner const &) = delete;
    Owner(Owner && o) noexcept : raw(std::exchange(o.raw, nullptr)) {}
    Owner & operator=(Owner && o) noexcept
    {
        std::swap(raw, o.raw);
        return *this;
    }
    ~Owner() { reset(); }
    void reset()
    {
        if (raw)
            (void)kRelease(std::exchange(raw, nullptr));
    }
    T * out() // where a create call writes (what was held goes first)
    {
        reset();
        return &raw;
    }
    operator T() const { return raw; }
};
using Event  = Owner<hipEvent_t, hipEventDestroy>;
using Stream = Owner<hipStream_t, hipStreamDestroy>;
template <class T>
using DevBlock = Owner<T *, hipFree>;
template <class T>
using PinnedBlock = Owner<T *, hipHostFree>;

static_assert(!std::is_copy_constructible<DevBuf>::value && !std::is_copy_assignable<DevBuf>::value, "DevBuf owns its block");
static_assert(!std::is_copy_constructible<Pinned>::value && !std::is_copy_assignable<Pinned>::value, "Pinned owns its block");
static_assert(!std::is_copy_constructible<Event>::value && !std::is_copy_assignable<Event>::value, "Event owns its event");
static_assert(!std::is_copy_constructible<Stream>::value && !std::is_copy_assignable<Stream>::value, "Stream owns its stream");
static_assert(!std::is_copy_constructible<DevBlock<int>>::value && !std::is_copy_constructible<PinnedBlock<int>>::value, "a block has one owner");
static_assert(std::is_nothrow_move_constructible<Event>::value && std::is_nothrow_move_constructible<DevBuf>::value, "owners move (std::vector<Event>)");

// Room for `bytes` in b (lx_handle.cpp).  A block that is too small is given back and a larger one taken: what it held is gone.
// ensure waits for the device first (kernels on a caller's stream may still read the old block) and leaves room to grow into.
int ensure(lx_handle * h, DevBuf & b, size_t bytes);
// A pinned block takes exactly `bytes` (kExact: the lanes of the BGZF and gunzip chunks, whose sizes have a fixed ceiling) or a quarter
// more and 4096 (kRoom: the staging of the pipelines and of Level 2, which follows the lists); flags: hipHostMalloc's.
enum PinGrowth
{
    kExact,
    kRoom
};
int ensure_pinned(lx_handle * h, Pinned & b, size_t bytes, PinGrowth growth, unsigned flags = hipHostMallocDefault);

} // namespace lxi
