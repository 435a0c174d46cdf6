// plugin_common.h -- helpers shared by the nvImageCodec plugin objects of this extension.
#pragma once
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/nvimgcodec_abi.h"
#include "staging.h"

namespace hipjpeg_ext {

constexpr const char* kExtensionId = "hipjpeg_ext";
constexpr const char* kDecoderId = "hipjpeg_decoder";
constexpr const char* kEncoderId = "hipjpeg_encoder";
constexpr uint32_t kExtensionVersion = NVIMGCODEC_MAKE_VERSION(0, 1, 0);

// Logging goes through the framework's log hook (reference extensions/libjpeg_turbo/log.h:30-40).
inline void log_message(const nvimgcodecFrameworkDesc_t* fw, const char* codec_id, nvimgcodecDebugMessageSeverity_t severity,
                        const std::string& msg)
{
    if (!fw || !fw->log) return;
    nvimgcodecDebugMessageData_t data{NVIMGCODEC_STRUCTURE_TYPE_DEBUG_MESSAGE_DATA, sizeof(nvimgcodecDebugMessageData_t), nullptr,
                                      msg.c_str(), 0, "jpeg", codec_id, kExtensionVersion};
    fw->log(fw->instance, severity, NVIMGCODEC_DEBUG_MESSAGE_CATEGORY_GENERAL, &data);
}

#define HJ_LOG(fw, id, sev, expr)                              \
    do {                                                       \
        std::ostringstream _ss;                                \
        _ss << expr;                                           \
        ::hipjpeg_ext::log_message(fw, id, sev, _ss.str());    \
    } while (0)
#define HJ_LOG_ERROR(fw, id, expr) HJ_LOG(fw, id, NVIMGCODEC_DEBUG_MESSAGE_SEVERITY_ERROR, expr)
#define HJ_LOG_WARNING(fw, id, expr) HJ_LOG(fw, id, NVIMGCODEC_DEBUG_MESSAGE_SEVERITY_WARNING, expr)
#define HJ_LOG_DEBUG(fw, id, expr) HJ_LOG(fw, id, NVIMGCODEC_DEBUG_MESSAGE_SEVERITY_DEBUG, expr)
#define HJ_LOG_TRACE(fw, id, expr) HJ_LOG(fw, id, NVIMGCODEC_DEBUG_MESSAGE_SEVERITY_TRACE, expr)

// "<module>:<key>=<value> ..." option strings; an empty module applies to every plugin
// (same grammar as extensions/libjpeg_turbo/libjpeg_turbo_decoder.cpp:250-276).
template <typename F>
inline void for_each_option(const char* options, const char* module_name, F&& fn, std::vector<std::string>* addressed = nullptr)
{
    std::istringstream iss(options ? options : "");
    std::string token;
    while (std::getline(iss, token, ' ')) {
        auto colon = token.find(':');
        auto equal = token.find('=');
        if (colon == std::string::npos || equal == std::string::npos || colon > equal) continue;
        std::string module = token.substr(0, colon);
        if (!module.empty() && module != module_name) continue;
        if (addressed && !module.empty()) addressed->push_back(token.substr(colon + 1, equal - colon - 1));  // named this very module
        fn(token.substr(colon + 1, equal - colon - 1), token.substr(equal + 1));
    }
}

// The execution parameters' device / pinned allocators as allocation hooks of the batches (an allocator needs both functions).
inline hipjpeg::MemoryHooks memory_hooks(const nvimgcodecExecutionParams_t* ep)
{
    hipjpeg::MemoryHooks hooks;
    if (ep->device_allocator && ep->device_allocator->device_malloc && ep->device_allocator->device_free) {
        hooks.device_malloc = reinterpret_cast<int (*)(void*, void**, size_t, void*)>(ep->device_allocator->device_malloc);
        hooks.device_free = reinterpret_cast<int (*)(void*, void*, size_t, void*)>(ep->device_allocator->device_free);
        hooks.device_ctx = ep->device_allocator->device_ctx;
    }
    if (ep->pinned_allocator && ep->pinned_allocator->pinned_malloc && ep->pinned_allocator->pinned_free) {
        hooks.pinned_malloc = reinterpret_cast<int (*)(void*, void**, size_t, void*)>(ep->pinned_allocator->pinned_malloc);
        hooks.pinned_free = reinterpret_cast<int (*)(void*, void*, size_t, void*)>(ep->pinned_allocator->pinned_free);
        hooks.pinned_ctx = ep->pinned_allocator->pinned_ctx;
    }
    return hooks;
}

// Walks a struct_next chain looking for a given structure type.
template <typename T>
inline T* find_in_chain(void* next, nvimgcodecStructureType_t type)
{
    struct Head {
        nvimgcodecStructureType_t struct_type;
        size_t struct_size;
        void* struct_next;
    };
    Head* h = static_cast<Head*>(next);
    while (h && h->struct_type != type) h = static_cast<Head*>(h->struct_next);
    return reinterpret_cast<T*>(h);
}

// An image info struct as getImageInfo wants to be handed one: zeroed, typed, sized, `next` chained behind it.
inline void init_info(nvimgcodecImageInfo_t* info, void* next = nullptr)
{
    memset(info, 0, sizeof *info);
    info->struct_type = NVIMGCODEC_STRUCTURE_TYPE_IMAGE_INFO;
    info->struct_size = sizeof *info;
    info->struct_next = next;
}

// What a code stream says it is: its image info with the JPEG info struct chained behind it (encoding UNKNOWN where the stream fills none).
inline nvimgcodecStatus_t stream_info(nvimgcodecCodeStreamDesc_t* cs, nvimgcodecImageInfo_t* cs_info, nvimgcodecJpegImageInfo_t* jpeg_info)
{
    *jpeg_info = nvimgcodecJpegImageInfo_t{NVIMGCODEC_STRUCTURE_TYPE_JPEG_IMAGE_INFO, sizeof(nvimgcodecJpegImageInfo_t), nullptr,
                                           NVIMGCODEC_JPEG_ENCODING_UNKNOWN};
    init_info(cs_info, jpeg_info);
    return cs->getImageInfo(cs->instance, cs_info);
}

}  // namespace hipjpeg_ext
