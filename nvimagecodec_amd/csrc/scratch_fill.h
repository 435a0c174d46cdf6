// scratch_fill.h -- what the host twins of the GPU algorithms (gpu_huffman_host.cpp, progressive_gpu_host.cpp, lossless_gpu_host.cpp,
// gpu_huffman_encode_host.cpp, progressive_encode_host.cpp, lossless_encode_host.cpp) take where the device takes a region of a staging arena.
//
// The arenas (staging.h) are never cleared as a whole: a kernel may read only what an earlier copy, memset or kernel of the same batch
// wrote (docs/arena_regions.md).  A twin that value-initialises its vectors would agree with the kernels only over zeroed memory, which
// the device never promises.  So every vector of a twin that stands for device scratch comes from device_scratch(): filled with the byte
// of hipjpegTestSetScratchFill (0 by default: the bytes a value-initialised vector has).  Where the device path really clears a region
// (a hipMemsetAsync, a clearing kernel, zeroed LDS) the twin keeps its own zero and names that clear in a comment.
#pragma once
#include <atomic>
#include <cstddef>
#include <cstring>
#include <type_traits>
#include <vector>

namespace hipjpeg {

inline std::atomic<int>& scratch_fill_byte()
{
    static std::atomic<int> byte{0};
    return byte;
}

template <class T>
std::vector<T> device_scratch(size_t n)
{
    static_assert(std::is_trivially_copyable<T>::value, "scratch is bytes");
    std::vector<T> v(n);
    if (n) memset(static_cast<void*>(v.data()), scratch_fill_byte().load(std::memory_order_relaxed), n * sizeof(T));
    return v;
}

// the same for memory the caller owns and the device would have taken from an arena (the coefficient blocks of a GPU-decoded picture)
inline void fill_device_scratch(void* p, size_t bytes)
{
    if (bytes) memset(p, scratch_fill_byte().load(std::memory_order_relaxed), bytes);
}

}  // namespace hipjpeg
