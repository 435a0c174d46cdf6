// staging.cpp -- see staging.h
#include "staging.h"

#include <hip/hip_runtime_api.h>

namespace hipjpeg {

hipjpegStatus_t Buffer::reserve(size_t bytes)
{
    if (bytes <= cap_) return HIPJPEG_STATUS_SUCCESS;
    release();
    size_t want = align_up(bytes + bytes / 8, 1 << 20);  // headroom so a slightly bigger next batch does not reallocate
    void* p = nullptr;
    if (hooks_) hooks_->used.store(true);
    if (kind_ == kDevice && hooks_ && hooks_->device_malloc) {
        if (hooks_->device_malloc(hooks_->device_ctx, &p, want, nullptr) != 0 || !p) return HIPJPEG_STATUS_ALLOC_FAILED;
        custom_ = true;
    } else if (kind_ == kPinned && hooks_ && hooks_->pinned_malloc) {
        if (hooks_->pinned_malloc(hooks_->pinned_ctx, &p, want, nullptr) != 0 || !p) return HIPJPEG_STATUS_ALLOC_FAILED;
        custom_ = true;
    } else {
        hipError_t e = kind_ == kDevice ? hipMalloc(&p, want) : hipHostMalloc(&p, want, hipHostMallocDefault);
        if (e != hipSuccess) return HIPJPEG_STATUS_ALLOC_FAILED;
        custom_ = false;
    }
    ptr_ = static_cast<uint8_t*>(p);
    cap_ = want;
    return HIPJPEG_STATUS_SUCCESS;
}

void Buffer::release()
{
    if (!ptr_) return;
    if (custom_) {
        if (kind_ == kDevice)
            hooks_->device_free(hooks_->device_ctx, ptr_, cap_, nullptr);
        else
            hooks_->pinned_free(hooks_->pinned_ctx, ptr_, cap_, nullptr);
    } else if (kind_ == kDevice) {
        (void)hipFree(ptr_);
    } else {
        (void)hipHostFree(ptr_);
    }
    ptr_ = nullptr;
    cap_ = 0;
}

}  // namespace hipjpeg
