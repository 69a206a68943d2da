// encoded_slab.h — the owner of the device allocation behind encoded-blob handles (host.h: Encoded).
// K handles of a block point into ONE allocation (the slab: blob b's share at b * bstride); every handle is freed on its own and the
// slab goes with the last one.  A lone frieda_encode is the slab of one.  HIP-free: the free function is injected (the library's
// switches to the slab's device and calls hipFree; the CPU test counts), so the ownership logic runs without a GPU.
// The counter is atomic: handles of one slab may be freed from different threads.  (One handle is still one owner: freeing the
// same handle twice is the caller's error, as before.)
#pragma once
#include <stdint.h>

#include <atomic>

namespace frieda {

struct EncodedSlab {
    void* base;
    int device;
    void (*free_fn)(void* base, int device);
    std::atomic<uint32_t> handles;  // handles still alive
};

// `handles` references are handed out at once: one per handle the caller is about to make
inline EncodedSlab* slab_create(void* base, int device, uint32_t handles, void (*free_fn)(void*, int)) {
    return new EncodedSlab{base, device, free_fn, {handles}};
}

// one handle lets go; true: it was the last one, the allocation was freed (free_fn ran, exactly once) and `s` is gone
inline bool slab_drop(EncodedSlab* s) {
    // acq_rel: everything the other handles' threads did before their drop happens before the free
    if (s->handles.fetch_sub(1, std::memory_order_acq_rel) != 1) return false;
    s->free_fn(s->base, s->device);
    delete s;
    return true;
}

}  // namespace frieda
