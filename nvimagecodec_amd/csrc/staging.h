// staging.h -- the memory every batch (decode and encode) stages its tables in: grow-only device / pinned buffers, allocated
// through the caller's hooks when there are any, and the bump allocator that lays out an arena inside one of them.
#pragma once
#include <atomic>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/hipjpeg.h"

namespace hipjpeg {

// Custom allocation hooks (the plugin forwards nvimgcodecDeviceAllocator_t / nvimgcodecPinnedAllocator_t here).
struct MemoryHooks {
    int (*device_malloc)(void* ctx, void** ptr, size_t size, void* stream) = nullptr;
    int (*device_free)(void* ctx, void* ptr, size_t size, void* stream) = nullptr;
    void* device_ctx = nullptr;
    int (*pinned_malloc)(void* ctx, void** ptr, size_t size, void* stream) = nullptr;
    int (*pinned_free)(void* ctx, void* ptr, size_t size, void* stream) = nullptr;
    void* pinned_ctx = nullptr;
    // Set by the first Buffer that allocates with these hooks (any kind, custom or not): from then on the functions may not change,
    // or a buffer would be handed back to another allocator than the one it came from (hipjpegSetAllocators).
    mutable std::atomic<bool> used{false};
    MemoryHooks() = default;
    MemoryHooks(const MemoryHooks& o)
        : device_malloc(o.device_malloc), device_free(o.device_free), device_ctx(o.device_ctx), pinned_malloc(o.pinned_malloc),
          pinned_free(o.pinned_free), pinned_ctx(o.pinned_ctx), used(o.used.load())
    {
    }
    MemoryHooks& operator=(const MemoryHooks&) = delete;
};

class Buffer {
public:
    enum Kind { kDevice, kPinned };
    Buffer(Kind kind, const MemoryHooks* hooks) : kind_(kind), hooks_(hooks) {}
    ~Buffer() { release(); }
    Buffer(const Buffer&) = delete;
    Buffer& operator=(const Buffer&) = delete;
    // grow-only; contents are NOT preserved
    hipjpegStatus_t reserve(size_t bytes);
    void release();
    uint8_t* data() const { return ptr_; }
    size_t capacity() const { return cap_; }
    bool custom() const { return custom_; }  // allocated through the caller's hooks

private:
    Kind kind_;
    const MemoryHooks* hooks_;
    uint8_t* ptr_ = nullptr;
    size_t cap_ = 0;
    bool custom_ = false;
};

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Bump allocator over one arena: every region starts at the next multiple of `align` behind the one taken before it.
struct Carve {
    size_t end = 0;
    size_t take(size_t bytes, size_t align = 256)
    {
        end = (end + align - 1) / align * align + bytes;
        return end - bytes;
    }
};

// The arenas hold every table at a byte offset: this is the one typed view of such a table.
template <class T>
T* at(const Buffer& b, size_t offset) { return reinterpret_cast<T*>(b.data() + offset); }
template <class T>
void copy_table(const Buffer& b, size_t offset, const std::vector<T>& v) { if (!v.empty()) memcpy(b.data() + offset, v.data(), v.size() * sizeof(T)); }

}  // namespace hipjpeg
