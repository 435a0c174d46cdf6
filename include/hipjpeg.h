/*
 * hipjpeg.h -- C-ABI of the MI355X-native JPEG hot path (libhipjpeg_ext.so).
 *
 * Plain pointers and sizes only; no C++ or torch types.  These are the entry points a host-language binding
 * (ctypes / cgo / JNI ...) uses, and the same library also exports the nvImageCodec plugin entry symbol
 * `nvimgcodecExtensionModuleEntry` (include/nvimgcodec_abi.h) through which an unmodified nvImageCodec loads it.
 *
 * Each group of functions names the reference interface it replaces (paths relative to /root/reference):
 *
 *   hipjpegGetImageInfo          nvjpegJpegStreamParse(Header)       extensions/nvjpeg/cuda_decoder.cpp:503-504,
 *                                / the framework's JPEG parser       src/parsers/jpeg.cpp:202-361
 *   hipjpegEntropyDecodeHost     nvjpegDecodeJpegHost                extensions/nvjpeg/cuda_decoder.cpp:527-530
 *   hipjpegDecodeBatch*          nvjpegDecodeJpegTransferToDevice +  extensions/nvjpeg/cuda_decoder.cpp:544-549
 *                                nvjpegDecodeJpegDevice               (one batched launch instead of one per image)
 *   hipjpegEncodeBatch*          nvjpegEncodeImage/RetrieveBitstream extensions/nvjpeg/cuda_encoder.cpp:362-381
 *
 * All device pointers are ordinary HIP device allocations; `stream` is a hipStream_t passed as void*.
 * Every function returns hipjpegStatus_t (0 = success).  The library never falls back to a CPU pixel path:
 * if no HIP device is usable, the device entry points return HIPJPEG_STATUS_NO_DEVICE.
 */
#ifndef HIPJPEG_H_
#define HIPJPEG_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HIPJPEG_API __attribute__((visibility("default")))

typedef enum {
    HIPJPEG_STATUS_SUCCESS = 0,
    HIPJPEG_STATUS_INVALID_ARGUMENT = 1,
    HIPJPEG_STATUS_BAD_JPEG = 2,         /* not a JPEG or malformed marker segment */
    HIPJPEG_STATUS_UNSUPPORTED = 3,      /* valid JPEG outside the entry point's scope (arithmetic, 12-bit DCT, hierarchical, ...; a lossless
                                            frame anywhere but in the hipjpeg*Lossless* calls, and there one outside their rules) */
    HIPJPEG_STATUS_TRUNCATED = 4,        /* entropy-coded data ends early */
    HIPJPEG_STATUS_CORRUPT = 5,          /* invalid Huffman code / restart marker / coefficient index */
    HIPJPEG_STATUS_ALLOC_FAILED = 6,
    HIPJPEG_STATUS_HIP_ERROR = 7,
    HIPJPEG_STATUS_NO_DEVICE = 8,
    HIPJPEG_STATUS_BUFFER_TOO_SMALL = 9,
    HIPJPEG_STATUS_INTERNAL_ERROR = 10   /* a C++ exception was caught at the C boundary (never propagated to the caller) */
} hipjpegStatus_t;

/* Output pixel layouts; numeric values equal hipjpeg::OutFormat (csrc/device_layout.h). They correspond to
 * nvimgcodecSampleFormat_t I_RGB, I_BGR, P_RGB, P_BGR, P_Y, P_YUV (type_convert.cpp:19-41 in the reference). */
typedef enum {
    HIPJPEG_OUTPUT_RGBI = 0,
    HIPJPEG_OUTPUT_BGRI = 1,
    HIPJPEG_OUTPUT_RGB_PLANAR = 2,
    HIPJPEG_OUTPUT_BGR_PLANAR = 3,
    HIPJPEG_OUTPUT_Y = 4,
    HIPJPEG_OUTPUT_YUV_PLANAR = 5
} hipjpegOutputFormat_t;

typedef enum {
    HIPJPEG_CSS_444 = 0,
    HIPJPEG_CSS_422 = 1,
    HIPJPEG_CSS_420 = 2,
    HIPJPEG_CSS_440 = 3,
    HIPJPEG_CSS_411 = 4,
    HIPJPEG_CSS_410 = 5,
    HIPJPEG_CSS_GRAY = 6,
    HIPJPEG_CSS_410V = 7,
    HIPJPEG_CSS_UNKNOWN = -1
} hipjpegChromaSubsampling_t;

#define HIPJPEG_FLAG_FANCY_UPSAMPLING 1u /* libjpeg do_fancy_upsampling (plugin option fancy_upsampling, default on) */
#define HIPJPEG_FLAG_GPU_HUFFMAN 2u      /* entropy-decode eligible streams on the GPU (sequential Huffman in up to 4 scans that code every
                                            component once, in any component order, each scan a stream of its own, with or without restart
                                            intervals; progressive SOF2 with up to 24 scans); the host then only finds the scans.  Other
                                            streams keep the host entropy stage -- progressive files with restart intervals among them,
                                            unless HIPJPEG_FLAG_GPU_PROGRESSIVE_INTERVALS is set too.  Encoding: entropy-code on the GPU every image without a
                                            restart interval -- baseline with Annex-K or optimized tables, or progressive output -- see
                                            hipjpegEncodeBatchEntropy; images with a restart interval stay with the host coder unless
                                            HIPJPEG_FLAG_GPU_RESTART_INTERVALS is set too. */
#define HIPJPEG_FLAG_FAST_IDCT 4u        /* the fast integer IDCT (plugin option hipjpeg_decoder:fast_idct=1; the reference's fast_idct, which
                                            selects JDCT_IFAST): the pixels are those of libjpeg-turbo's x86-64 SIMD routine
                                            jsimd_idct_ifast_sse2, which differs from jidctfst.c only on streams whose samples leave the
                                            gamut.  Without the flag: JDCT_ISLOW (jsimd_idct_islow), the library's default. */
#define HIPJPEG_FLAG_GPU_PROGRESSIVE_INTERVALS 16u /* decoding, together with HIPJPEG_FLAG_GPU_HUFFMAN (alone it means nothing): progressive
                                            files in which EVERY scan has a restart interval take the GPU entropy stage too, a lane per
                                            restart interval (csrc/progressive_interval_core.h).  Rules: those of progressive files without
                                            restart intervals, and every scan's interval is 1..65535 with each interval but the last closed by
                                            its marker, and the AC scans of a component share one interval; other such files keep the host
                                            entropy stage.  Honoured by hipjpegDecodeBatch / Host / Submit, hipjpegDecodeCoefficientsBatch and
                                            hipjpegTranscodeBatch; plugin option hipjpeg_decoder:gpu_progressive_intervals=1.  Default off:
                                            without it such files decode on the host entropy stage as before.  (8u is
                                            HIPJPEG_FLAG_GPU_RESTART_INTERVALS of the coder, ignored when decoding.) */

typedef struct {
    int32_t width, height, num_components;
    int32_t sof_marker;  /* 0xC0 baseline, 0xC1 extended, 0xC2 progressive, other = unsupported type */
    int32_t color_model; /* 0 gray, 1 YCbCr, 2 RGB, 3 CMYK, 4 YCCK */
    int32_t subsampling; /* hipjpegChromaSubsampling_t */
    int32_t restart_interval, num_scans;
    int32_t h[4], v[4];
    int32_t blocks_w[4], blocks_h[4]; /* MCU-padded block grid per component */
    int32_t samp_w[4], samp_h[4];     /* true component size in samples */
    uint64_t coef_bytes;              /* bytes of int16 coefficient storage for the whole image */
} hipjpegImageInfo_t;

typedef struct {
    void* plane[3];     /* device pointers; interleaved formats use plane[0] only */
    uint32_t pitch[3];  /* bytes per row */
} hipjpegOutput_t;

/* Optional per-image geometry: region of interest and EXIF orientation, applied on the device after decoding.
 * The output buffer then holds the region (all zeros = whole image) of the decoded image, brought upright according to
 * `orientation` (EXIF tag 0x0112 values 1..8; 0 or 1 = leave as stored): its size is (x1-x0) x (y1-y0), swapped for
 * orientations 5..8.  Mirrors nvimgcodecImageInfo_t::region (ref include/nvimgcodec.h:446-455; crop semantics of
 * extensions/libjpeg_turbo/jpeg_mem.cpp:206-240: exactly the pixels of the full decode) and nvimgcodecOrientation_t as the
 * nvJPEG plugin applies it (ref extensions/nvjpeg/cuda_decoder.cpp:443-478, type_convert.cpp:43-64).
 * Not available for HIPJPEG_OUTPUT_YUV_PLANAR (subsampled planes): such images report HIPJPEG_STATUS_UNSUPPORTED. */
typedef struct {
    int32_t x0, y0, x1, y1; /* region in stored-image coordinates, end exclusive */
    int32_t orientation;    /* EXIF orientation 1..8 (0 = 1) */
} hipjpegTransform_t;

typedef struct hipjpegHandle* hipjpegHandle_t;

HIPJPEG_API const char* hipjpegStatusString(hipjpegStatus_t status);
HIPJPEG_API int hipjpegVersion(void);
/* ---- test hooks.  Every hipjpegTest* entry point answers only in a process started with HIPJPEG_ENABLE_TEST_HOOKS=1 (read once) and
 * refuses (INVALID_ARGUMENT / -1) anywhere else: a production process cannot have a throw armed inside the library. ---- */
/* Test hook (fault injection): the `countdown`-th passage of the named host-code site from now on throws a C++ exception
 * inside the library, once; site NULL or "" disarms.  Sites: "plan", "entropy_stage", "finalize", "transfer", "launch",
 * "resolve", "marshal".  The boundary must turn it into a status code / per-sample FAIL; tests/test_gpu_plugin.py relies on it. */
HIPJPEG_API hipjpegStatus_t hipjpegTestSetFault(const char* site, int countdown);
/* Test hook: how many times a plugin has reported a sample that had already been reported (must stay 0: exactly one
 * imageReady per sample, reference src/processing_results.cpp:104-115). Counted by this library's host harness. */
HIPJPEG_API int hipjpegTestDoubleReports(void);
/* Test hook: how many images of the handle's last settled batch the GPU entropy stage handed back to the host entropy decoder
 * (damaged streams, and periodic streams whose corrections would have to travel through the image subsequence by subsequence). */
HIPJPEG_API int32_t hipjpegTestHostFallbacks(hipjpegHandle_t handle);
/* Test hook: work units of the handle's current batch per kernel -- plane_units[0]: the plane IDCT kernel (K1); luma_units[3]: the fused
 * luma kernel (K2) by layout (0 generic, 1 the everyday interleaved kernel, 2 the everyday planar kernel; csrc/decode_kernels.h). */
HIPJPEG_API hipjpegStatus_t hipjpegTestKernelFlavours(hipjpegHandle_t handle, int32_t plane_units[1], int32_t luma_units[3]);
/* Test hook: how many of those work units went to the FUSED kernel builds (blocks Huffman-decoded inside the pixel kernels,
 * HIPJPEG_FUSED_DECODE=1); negative without a handle. */
HIPJPEG_API int32_t hipjpegTestFusedUnits(hipjpegHandle_t handle);

/* Test hook (host only): the parser's per-chunk counts of the bytes that byte-stuffing removal drops from scan `scan_index` (16,384-byte
 * chunks of the entropy-coded segment; the GPU entropy stage's compact kernel works from them).  Returns the number of chunks, or a
 * negative value when the file does not parse / has no such scan; at most `capacity` counts are written. */
HIPJPEG_API int32_t hipjpegTestScanChunkDrops(const uint8_t* data, size_t length, int scan_index, uint32_t* drops, int32_t capacity);
/* Test hook (host only): the steps the GPU entropy stage's position walks take over one AC Huffman table (bits[16], vals[nvals] as in
 * a DHT segment), from the table's first-level and pair entries: steps[w * 64 + z] for every 10-bit window w and zigzag position z =
 * bits consumed | zigzag advance << 8 | (two symbols taken as a pair) << 16 | (w opens a code longer than 10 bits) << 17.
 * steps: 65,536 entries.  Returns 0, or a negative value for a table the stage does not accept. */
HIPJPEG_API int32_t hipjpegTestPairSteps(const uint8_t bits[16], const uint8_t* vals, int32_t nvals, uint32_t* steps);

/* Test hook (host only): how much the first synchronisation launch of the GPU entropy stage decodes, counted by the host twin
 * (hipjpegEntropyDecodeGpuAlgorithmHost, whose self-checks run as well and answer INTERNAL_ERROR) for both of its schedules, summed over
 * the file's scans.  counts[0..4]: one sync unit per workgroup -- subsequence decodes of pass 0, 0, of correction round 1, of round 2,
 * and the tasks left for the tail kernel behind round 2.  counts[5..9]: two units per workgroup, the schedule the kernels run -- decodes
 * of phase A (even rows from the assumed state), phase B (odd rows from their neighbour's end state), round 1, round 2, and the tasks
 * left for the tail kernel.  Halo rows count as decodes. */
HIPJPEG_API hipjpegStatus_t hipjpegTestSyncScheduleCounts(const uint8_t* data, size_t length, uint64_t counts[10]);

/* Test hook (host only): the byte the host twins of the GPU algorithms (hipjpegEntropyDecodeGpuAlgorithmHost,
 * hipjpegEntropyDecodeGpuIntervalAlgorithmHost, hipjpegLosslessEntropyAlgorithmHost, hipjpegEncodeBaselineGpuAlgorithmHost,
 * hipjpegEncodeProgressiveGpuAlgorithmHost) fill their stand-ins for device scratch with, 0..255, from now on and process-wide; 0 is the
 * default (csrc/scratch_fill.h).  Their results must not depend on it: a kernel reads nothing its batch did not write
 * (docs/arena_regions.md; tests/test_twin_scratch_fill.py). */
HIPJPEG_API hipjpegStatus_t hipjpegTestSetScratchFill(int byte);

/* ---- host-only entry points (usable without a GPU) ---- */
HIPJPEG_API hipjpegStatus_t hipjpegGetImageInfo(const uint8_t* data, size_t length, hipjpegImageInfo_t* info);

/* Huffman-decode every scan into quantized coefficient blocks in the device layout (block raster order per
 * component, 64 int16 per block stored column-major).  comp_offsets[c] receives the int16 offset of component c
 * inside `coef`; qtables[c*64 .. ] the (column-major) quantisation table of component c. */
HIPJPEG_API hipjpegStatus_t hipjpegEntropyDecodeHost(const uint8_t* data, size_t length, int16_t* coef, size_t coef_capacity_bytes,
                                                     uint64_t comp_offsets[4], uint16_t qtables[256]);

/* The host entropy stage's zero-run-compressed output (what crosses PCIe for host-decoded pictures since round 3; csrc/entropy_decode.h):
 * per-block offset tables (uint32 per block of each component's MCU-padded raster grid, the tables back to back; table_offsets[c] = index of
 * component c's first entry; 0 = block never coded) followed by the records [n : u8][DC : i16 LE] n x {position : u8, value : i16 LE}, position =
 * index into the device-layout block (column-major).  UNSUPPORTED for frames the format does not cover (progressive, several scans): those
 * stay dense.  capacity_bytes >= 200 bytes per block is always enough. */
HIPJPEG_API hipjpegStatus_t hipjpegEntropyDecodeHostSparse(const uint8_t* data, size_t length, uint8_t* stream, size_t capacity_bytes, size_t* stream_bytes,
                                                           uint64_t table_offsets[4]);

/* The GPU entropy decoder's algorithm (self-synchronizing subsequence decoding, csrc/huffman_gpu_core.h) executed on the
 * host, lane by lane, with the very code the kernels run: lets the algorithm be verified without a GPU.  Same output
 * layout as hipjpegEntropyDecodeHost; returns HIPJPEG_STATUS_UNSUPPORTED for streams the GPU entropy path does not take
 * (sequential streams in more than 4 scans or with a component that no scan or two scans code, arithmetic coding, progressive
 * scripts beyond the walker's limits), and
 * HIPJPEG_STATUS_INTERNAL_ERROR when one of its self-checks fails (a block-start record of the synchronisation decodes that
 * disagrees with the position walk). */
HIPJPEG_API hipjpegStatus_t hipjpegEntropyDecodeGpuAlgorithmHost(const uint8_t* data, size_t length, int16_t* coef,
                                                                 size_t coef_capacity_bytes, uint64_t comp_offsets[4],
                                                                 int32_t* sync_passes);

/* The algorithm of HIPJPEG_FLAG_GPU_PROGRESSIVE_INTERVALS (a lane per restart interval for the block start positions and the DC
 * planes, csrc/progressive_interval_core.h, then the replay of csrc/progressive_gpu_core.h) executed on the host with the very code the
 * kernels run.  Same output layout as hipjpegEntropyDecodeHost.  HIPJPEG_STATUS_UNSUPPORTED for everything the interval kernels do not
 * take: sequential streams, progressive files without restart intervals, a scan whose markers do not close every interval but the
 * last, AC scans of one component with different restart intervals.  hipjpegEntropyDecodeGpuAlgorithmHost keeps answering
 * UNSUPPORTED for progressive files with restart intervals. */
HIPJPEG_API hipjpegStatus_t hipjpegEntropyDecodeGpuIntervalAlgorithmHost(const uint8_t* data, size_t length, int16_t* coef,
                                                                         size_t coef_capacity_bytes, uint64_t comp_offsets[4]);

/* ---- device pipeline ---- */
/* num_host_threads: CPU threads for the entropy stage (0 = hardware concurrency). */
HIPJPEG_API hipjpegStatus_t hipjpegCreate(hipjpegHandle_t* handle, int device_id, int num_host_threads);
HIPJPEG_API hipjpegStatus_t hipjpegDestroy(hipjpegHandle_t handle);

/* Caller-supplied allocators for everything the handle stages its batches in (the grow-only device and pinned arenas of its decode pages,
 * encode batch and encode pages, lossless pages, and through them the transcode and coefficient calls) -- what the plugin takes from
 * nvimgcodecExecutionParams_t::device_allocator / pinned_allocator (reference include/nvimgcodec.h, nvimgcodecDeviceAllocator_t /
 * nvimgcodecPinnedAllocator_t: the same signatures).  malloc returns 0 and a pointer in *ptr on success; free gets the size malloc was
 * asked for; `stream` is always NULL (the arenas are allocated and released outside any stream order).  A pair counts only when both of
 * its functions are set; either pair may be null, and that kind of memory then comes from hipMalloc / hipHostMalloc as before.  The
 * memory need not be cleared: nothing a kernel reads from an arena before its own batch wrote it can reach an output, a status or an
 * address (docs/arena_regions.md).  Device
 * scratch that is not an arena (a few words the entropy stage allocates once per handle) stays with hipMalloc. */
typedef struct {
    int (*device_malloc)(void* ctx, void** ptr, size_t size, void* stream);
    int (*device_free)(void* ctx, void* ptr, size_t size, void* stream);
    void* device_ctx;
    int (*pinned_malloc)(void* ctx, void** ptr, size_t size, void* stream);
    int (*pinned_free)(void* ctx, void* ptr, size_t size, void* stream);
    void* pinned_ctx;
} hipjpegAllocators_t;
/* Accepted only before the handle's first batch of any kind (nothing has been allocated yet); afterwards, or with a null argument,
 * HIPJPEG_STATUS_INVALID_ARGUMENT and nothing changes.  The functions and contexts must stay valid until hipjpegDestroy, which hands
 * every allocation back. */
HIPJPEG_API hipjpegStatus_t hipjpegSetAllocators(hipjpegHandle_t handle, const hipjpegAllocators_t* allocators);

/* One call = host entropy stage (thread pool) + H2D staging + batched device stage, asynchronous on `stream`
 * (the call returns after the last kernel is enqueued; per-image host failures are reported in `statuses`).  With
 * HIPJPEG_FLAG_GPU_HUFFMAN and at least one image on the GPU entropy stage the call then WAITS on `stream` for that stage's verdicts,
 * and so for everything queued on `stream` before it: `statuses` are final when it returns.  Either way the outputs are written in
 * the order of `stream` and by nothing else: not before the work queued on it earlier, and visible to the work queued on it later. */
HIPJPEG_API hipjpegStatus_t hipjpegDecodeBatch(hipjpegHandle_t handle, const uint8_t* const* data, const size_t* lengths, int batch_size,
                                               const hipjpegOutput_t* outputs, hipjpegOutputFormat_t format, unsigned flags,
                                               hipjpegStatus_t* statuses, void* stream);

/* Geometry for the NEXT batch handed to hipjpegDecodeBatch / Host / Submit or to hipjpegCoefficientsToPixelsBatch: `transforms` =
 * batch_size entries (copied), or NULL to go back to plain decoding.  Consumed by that one batch. */
HIPJPEG_API hipjpegStatus_t hipjpegDecodeBatchSetTransforms(hipjpegHandle_t handle, const hipjpegTransform_t* transforms, int batch_size);

/* Decoding at 1/2, 1/4 or 1/8 scale: libjpeg's scale_num / scale_denom = 1 / denominator (the reference's UncompressFlags::ratio), a smaller
 * IDCT per block.  Host only: the size of a width x height picture decoded at 1 / scale_denom -- ceil(extent * (8 / scale_denom) / 8), what
 * libjpeg-turbo reports as output_width / output_height.  Denominators 1, 2, 4, 8; anything else is HIPJPEG_STATUS_INVALID_ARGUMENT. */
HIPJPEG_API hipjpegStatus_t hipjpegGetScaledImageSize(int32_t width, int32_t height, int32_t scale_denom, int32_t* scaled_width,
                                                      int32_t* scaled_height);
/* Scale denominators for the NEXT batch handed to hipjpegDecodeBatch / Host / Submit: `scale_denoms` = batch_size entries (copied), or NULL
 * for none.  Consumed by that one batch; a count other than that batch's size makes that call HIPJPEG_STATUS_INVALID_ARGUMENT.  Per image:
 * 1 = today's path and bytes; 2, 4, 8 = the picture libjpeg-turbo decodes with that scale_denom, bit for bit (tests/golden/
 * manifest_scaled.json), written by kernels of their own; any other value gives that image HIPJPEG_STATUS_INVALID_ARGUMENT.  Outputs,
 * pitches and transforms of a scaled image are judged at its scaled size (hipjpegGetScaledImageSize), and the region of a
 * hipjpegTransform_t is in scaled-picture coordinates.  HIPJPEG_FLAG_FAST_IDCT then reaches only the components libjpeg still gives the
 * full 8x8 transform (the chroma of a 4:2:0 file at 1/2); the 4x4, 2x2 and 1x1 transforms have one arithmetic.
 * HIPJPEG_FLAG_FANCY_UPSAMPLING filters what is left to upsample, except at 1/8, where libjpeg replicates.  HIPJPEG_STATUS_UNSUPPORTED for
 * a scaled image: HIPJPEG_OUTPUT_YUV_PLANAR and four-component frames.  hipjpegCoefficientsToPixelsBatch, hipjpegDecodeCoefficientsBatch
 * and hipjpegTranscodeBatch take no scales: called with scales pending they return HIPJPEG_STATUS_INVALID_ARGUMENT and drop them.
 * Scaled images never take the FUSED kernel builds (the HIPJPEG_FUSED_DECODE=1 experiment, off by default), and because those builds are
 * all or nothing per batch, one scaled image puts the whole batch -- its denominator-1 images too -- on the default route, the block
 * pass through HBM: the same bytes, the default route's time. */
HIPJPEG_API hipjpegStatus_t hipjpegDecodeBatchSetScales(hipjpegHandle_t handle, const int32_t* scale_denoms, int batch_size);

/* The three phases separately (what hipjpegDecodeBatch does internally); used by bench.py to time the device
 * stage with the coefficient blocks already resident in HBM. */
HIPJPEG_API hipjpegStatus_t hipjpegDecodeBatchHost(hipjpegHandle_t handle, const uint8_t* const* data, const size_t* lengths, int batch_size,
                                                   const hipjpegOutput_t* outputs, hipjpegOutputFormat_t format, unsigned flags,
                                                   hipjpegStatus_t* statuses);
HIPJPEG_API hipjpegStatus_t hipjpegDecodeBatchTransfer(hipjpegHandle_t handle, void* stream);
HIPJPEG_API hipjpegStatus_t hipjpegDecodeBatchDevice(hipjpegHandle_t handle, void* stream);
/* One kernel family of the device stage at a time (0 = idct_plane, 1 = luma_color, 2 = generic_color, 3 = GPU entropy stage
 * followed by the blocking read-back of its verdicts, 4 = geometry pass, 6 = GPU entropy stage enqueued only: its verdicts
 * are settled by the next hipjpegDecodeBatchGetStatuses), so a caller can bracket each with events.  Any other `which` is
 * HIPJPEG_STATUS_INVALID_ARGUMENT.  hipjpegDecodeBatchDevice == entropy (if any image uses it), then 0, 1, 2, 4. */
HIPJPEG_API hipjpegStatus_t hipjpegDecodeBatchDeviceKernel(hipjpegHandle_t handle, int which, void* stream);
/* Pipelined submission.  Submit = host stage + H2D copy (on an internal copy stream) + every kernel on `stream`, without
 * waiting for anything on the device; at most three batches (hipjpegSetPipelineDepth: up to eight) may be in flight (the handle's staging pages).  Wait = block
 * until the OLDEST submitted batch has finished and return its final per-image statuses.  The host stage of batch n+1 and
 * its H2D copy overlap the kernels of batch n.  Outputs and `data` of a submitted batch must stay valid until its Wait. */
HIPJPEG_API hipjpegStatus_t hipjpegDecodeBatchSubmit(hipjpegHandle_t handle, const uint8_t* const* data, const size_t* lengths, int batch_size,
                                                     const hipjpegOutput_t* outputs, hipjpegOutputFormat_t format, unsigned flags, void* stream);
HIPJPEG_API hipjpegStatus_t hipjpegDecodeBatchWait(hipjpegHandle_t handle, hipjpegStatus_t* statuses, int batch_size);
/* Zero-copy input.  When an image's bitstream lies in page-locked host memory (hipHostMalloc / hipHostRegister, a pinned torch tensor) and
 * takes the GPU entropy stage, the copy engine reads the scan's bytes from THAT memory -- no staging copy on the host (one pass over host
 * DRAM per byte instead of three; what matters when eight ranks share a host).  Nothing to call: the library asks the runtime about every
 * input pointer; HIPJPEG_NO_ZERO_COPY=1 in the environment switches it off.  The caller keeps the memory valid until the batch has been
 * waited for (as for every Submit).  Returns how many images of the handle's current batch went that way (after Transfer / Submit). */
HIPJPEG_API int32_t hipjpegDecodeBatchZeroCopyImages(hipjpegHandle_t handle);
/* Images of the handle's current batch that took the interval kernels (HIPJPEG_FLAG_GPU_PROGRESSIVE_INTERVALS); they are counted among
 * the GPU-decoded images of hipjpegDecodeBatchEntropyStats too.  Negative without a handle. */
HIPJPEG_API int32_t hipjpegDecodeBatchIntervalImages(hipjpegHandle_t handle);
/* ... of which the interval kernels or the replay flagged (a stream they could not vouch for: damaged data) so that the host entropy
 * decoder decoded the image again and its verdict became the image's status.  Of the batch the last hipjpegDecodeBatchWait settled if no
 * batch has been planned since, else of the current batch once its statuses are final (hipjpegDecodeBatchGetStatuses, a blocking
 * hipjpegDecodeBatch / hipjpegDecodeCoefficientsBatch / hipjpegTranscodeBatch).  0 for undamaged files.  Negative without a handle. */
HIPJPEG_API int32_t hipjpegDecodeBatchIntervalTakeovers(hipjpegHandle_t handle);
/* What the current batch's transfer puts on PCIe (descriptors, tables, bitstreams of GPU-decoded pictures, coefficients of host-decoded ones)
 * and how many host-decoded pictures went as zero-run-compressed streams rather than dense blocks (HIPJPEG_DENSE_STAGING=1 switches that off). */
HIPJPEG_API hipjpegStatus_t hipjpegDecodeBatchTransferStats(hipjpegHandle_t handle, uint64_t* h2d_bytes, int32_t* sparse_images);

/* With HIPJPEG_FLAG_GPU_HUFFMAN: only images of MORE than `pixels` pixels (width x height) take the GPU entropy stage, smaller ones the
 * host Huffman decoder -- nvJPEG's switch between its HYBRID and GPU_HYBRID backends (plugin option hybrid_huffman_threshold,
 * reference extensions/nvjpeg/cuda_decoder.cpp:188-209, 512-521).  0 (default) = every eligible stream on the GPU. */
HIPJPEG_API hipjpegStatus_t hipjpegSetHybridHuffmanThreshold(hipjpegHandle_t handle, uint64_t pixels);

/* How many batches Submit may have in flight (staging pages in use): 1..8, default 3; only while nothing is in flight.
 * Batches of progressive images keep a small part of the chip busy for a long time (one wave per scan), so their throughput
 * grows with the depth; each page in flight runs its entropy stage on a stream of its own, and the HIP runtime must be
 * allowed as many hardware queues (environment GPU_MAX_HW_QUEUES, default 4, read when the runtime starts). */
HIPJPEG_API hipjpegStatus_t hipjpegSetPipelineDepth(hipjpegHandle_t handle, int depth);
/* Final per-image statuses of the current batch (after the device stage they include what the GPU entropy stage found;
 * blocks until that stage has reported). */
HIPJPEG_API hipjpegStatus_t hipjpegDecodeBatchGetStatuses(hipjpegHandle_t handle, hipjpegStatus_t* statuses, int batch_size);
/* GPU entropy stage statistics: images that used it, kernel launches the last synchronisation needed, destuffed bytes. */
HIPJPEG_API hipjpegStatus_t hipjpegDecodeBatchEntropyStats(hipjpegHandle_t handle, int32_t* gpu_images, int32_t* sync_launches,
                                                           uint64_t* stream_bytes);
/* Launch statistics of the prepared batch: workgroups per kernel (idct_plane, luma_color, generic). */
HIPJPEG_API hipjpegStatus_t hipjpegDecodeBatchStats(hipjpegHandle_t handle, int32_t num_units[3], uint64_t* coef_bytes,
                                                    uint64_t* output_bytes);

/* ---- encode: RGB -> baseline JPEG (replaces nvjpegEncodeImage + nvjpegEncodeRetrieveBitstream,
 *      reference extensions/nvjpeg/cuda_encoder.cpp:336-388) ---- */
typedef struct {
    const void* plane[3]; /* device pointers; interleaved / gray input uses plane[0] only */
    uint32_t pitch[3];
    int32_t width, height;
} hipjpegEncodeInput_t;

typedef struct {
    int32_t quality;           /* 1..100, libjpeg quality scaling of the Annex-K tables */
    int32_t subsampling;       /* hipjpegChromaSubsampling_t of the OUTPUT stream (GRAY = single component) */
    int32_t input_format;      /* HIPJPEG_OUTPUT_RGBI / BGRI / RGB_PLANAR / BGR_PLANAR / Y (gray plane) / YUV_PLANAR (Y, Cb, Cr planes
                                  already in the stream's sampling: plane c holds ceil(width / hs_c) x ceil(height / vs_c) samples) */
    int32_t restart_interval;  /* MCUs per restart interval, 0 = none */
    int32_t optimized_huffman; /* 0 = Annex-K tables, 1 = per-image optimal tables (two-pass) */
    int32_t progressive;       /* 0 = baseline sequential (SOF0); 1 = progressive (SOF2): libjpeg's jpeg_simple_progression scan script
                                  with per-scan optimal tables, what nvimgcodecJpegImageInfo_t::encoding = PROGRESSIVE_DCT_HUFFMAN asks
                                  for (reference extensions/nvjpeg/cuda_encoder.cpp:339-346) */
} hipjpegEncodeParams_t;
#define HIPJPEG_FLAG_GPU_RESTART_INTERVALS 8u /* encoding, together with HIPJPEG_FLAG_GPU_HUFFMAN in hipjpegEncodeBatchEntropy and
                                            hipjpegEncodeBatchSubmit: the GPU coder also takes baseline images (Annex-K or optimized tables)
                                            whose restart_interval is not 0.  Progressive output with a restart interval stays with the host
                                            coder unless HIPJPEG_FLAG_GPU_PROGRESSIVE_RESTART is set.  No meaning alone; the decode entry
                                            points ignore it. */
#define HIPJPEG_FLAG_GPU_PROGRESSIVE_RESTART 32u /* encoding, together with HIPJPEG_FLAG_GPU_HUFFMAN in hipjpegEncodeBatchEntropy,
                                            hipjpegEncodeBatchSubmit, hipjpegTranscodeBatch and hipjpegEncodeCoefficientsBatch: the GPU coder
                                            also takes progressive output whose restart_interval is not 0 (jcphuff.c emit_restart on the
                                            device: the EOB run flushed at every interval end, predictor reset, byte alignment, RSTn).
                                            Independent of HIPJPEG_FLAG_GPU_RESTART_INTERVALS, which keeps meaning baseline images only.
                                            No meaning alone; the decode entry points ignore it. */

/* Device stage only: colour conversion + downsampling + FDCT + quantization for the whole batch (asynchronous). */
HIPJPEG_API hipjpegStatus_t hipjpegEncodeBatchDevice(hipjpegHandle_t handle, const hipjpegEncodeInput_t* inputs,
                                                     const hipjpegEncodeParams_t* params, int batch_size, hipjpegStatus_t* statuses, void* stream);
/* Re-launch the kernel of the prepared batch (bench.py times this). */
HIPJPEG_API hipjpegStatus_t hipjpegEncodeBatchRelaunch(hipjpegHandle_t handle, void* stream);
/* D2H of the quantized coefficients, then Huffman coding + marker writing on the host thread pool (blocking). */
HIPJPEG_API hipjpegStatus_t hipjpegEncodeBatchHost(hipjpegHandle_t handle, hipjpegStatus_t* statuses);
/* Entropy stage with a choice: flags = HIPJPEG_FLAG_GPU_HUFFMAN codes every image without restart markers on the GPU: baseline with
 * Annex-K tables, or optimized ones (histograms on the device, jpeg_gen_optimal_table on the host, second pass on the device), and
 * progressive output (per-block summaries and the EOB-run resolution on the device, per-scan optimal tables on the host, then one
 * segment per scan; byte-identical to the host coder's SOF2 files); then lengths, prefix sums, bit packing, byte stuffing, file
 * assembly -- only finished JPEG files cross PCIe.  Images with a restart interval (which the reference's encode parameters do not have)
 * go through the host coder as in hipjpegEncodeBatchHost, and so does everything when flags = 0.  flags = HIPJPEG_FLAG_GPU_HUFFMAN |
 * HIPJPEG_FLAG_GPU_RESTART_INTERVALS: the GPU coder takes baseline images with a restart interval too (predictor reset, byte alignment
 * and RSTn markers on the device, the markers exempt from byte stuffing; byte-identical to the host coder's files); progressive output
 * with a restart interval still goes to the host coder unless HIPJPEG_FLAG_GPU_PROGRESSIVE_RESTART is set as well (or instead: the two
 * are independent), which sends it to the GPU coder with the same files.  Blocking. */
HIPJPEG_API hipjpegStatus_t hipjpegEncodeBatchEntropy(hipjpegHandle_t handle, unsigned flags, hipjpegStatus_t* statuses);
/* Both of the above. */
HIPJPEG_API hipjpegStatus_t hipjpegEncodeBatch(hipjpegHandle_t handle, const hipjpegEncodeInput_t* inputs, const hipjpegEncodeParams_t* params,
                                               int batch_size, hipjpegStatus_t* statuses, void* stream);
/* Pipelined encoding: Submit queues a whole batch (forward kernel + entropy stage per `flags` as in
 * hipjpegEncodeBatchEntropy + copy of the files to host memory) and returns at once; it runs on an internal stream, ordered
 * behind the work already queued on `stream` (the producer of the pixels).  Wait blocks until the OLDEST submitted batch is
 * complete, returns its statuses and makes it the batch hipjpegEncodeGetBitstream talks about.  At most three batches in
 * flight (three pages, used round robin); the bitstreams of a waited batch stay valid until a Submit takes its page again:
 * the third Submit after the one that queued it.  The PCIe-bound file output of one batch overlaps the kernels of the
 * others. */
HIPJPEG_API hipjpegStatus_t hipjpegEncodeBatchSubmit(hipjpegHandle_t handle, const hipjpegEncodeInput_t* inputs, const hipjpegEncodeParams_t* params,
                                                     int batch_size, unsigned flags, void* stream);
HIPJPEG_API hipjpegStatus_t hipjpegEncodeBatchWait(hipjpegHandle_t handle, hipjpegStatus_t* statuses, int batch_size);
/* Bitstream of image i of the last encoded (or waited-for) batch; valid until the next encode call on this handle. */
HIPJPEG_API hipjpegStatus_t hipjpegEncodeGetBitstream(hipjpegHandle_t handle, int index, const uint8_t** data, size_t* length);
/* Quantized coefficients of (image, component) after hipjpegEncodeBatchHost: zigzag-ordered int16[64] blocks over the
 * MCU-padded grid (only the real_w x real_h area is defined).  For tests and for callers with their own entropy coder. */
HIPJPEG_API hipjpegStatus_t hipjpegEncodeGetCoefficients(hipjpegHandle_t handle, int index, int component, const int16_t** coef,
                                                         int32_t grid[4] /* blocks_w, blocks_h, real_w, real_h */);
HIPJPEG_API hipjpegStatus_t hipjpegEncodeBatchStats(hipjpegHandle_t handle, int32_t* num_units, uint64_t* pixel_bytes, uint64_t* coef_bytes);
/* How many images of the handle's last entropy stage the GPU entropy coder took (baseline with Annex-K or optimized tables, and
 * progressive output; with a restart interval baseline images under HIPJPEG_FLAG_GPU_RESTART_INTERVALS and progressive ones under
 * HIPJPEG_FLAG_GPU_PROGRESSIVE_RESTART); the others were coded by the host coder. */
HIPJPEG_API int32_t hipjpegEncodeBatchGpuEntropyImages(hipjpegHandle_t handle);
/* Host-only: entropy-code given coefficient grids (zigzag order, MCU-padded grids as above) into a JFIF file.
 * Returns HIPJPEG_STATUS_BUFFER_TOO_SMALL with *length = needed size if capacity is insufficient. */
HIPJPEG_API hipjpegStatus_t hipjpegEncodeFromCoefficientsHost(int32_t width, int32_t height, const hipjpegEncodeParams_t* params,
                                                              const int16_t* const coef[3], uint8_t* out, size_t capacity, size_t* length);
/* The GPU entropy coder's progressive algorithm (csrc/progressive_encode_core.h: block summaries, EOB-run resolution, lengths, bit
 * emission) executed on the host, block by block, with the very code the kernels run: lets the algorithm be verified without a GPU.
 * Same signature and output as hipjpegEncodeFromCoefficientsHost; HIPJPEG_STATUS_UNSUPPORTED for what the GPU coder's progressive path
 * does not take without HIPJPEG_FLAG_GPU_PROGRESSIVE_RESTART (baseline output, restart intervals). */
HIPJPEG_API hipjpegStatus_t hipjpegEncodeFromCoefficientsGpuAlgorithmHost(int32_t width, int32_t height, const hipjpegEncodeParams_t* params,
                                                                          const int16_t* const coef[3], uint8_t* out, size_t capacity,
                                                                          size_t* length);
/* The same with any restart_interval (0..65535, 0 = none: the bytes of the function above): what the GPU coder's progressive path does
 * under HIPJPEG_FLAG_GPU_PROGRESSIVE_RESTART -- the interval-end flush of the EOB run, the segmented scan of the bit offsets, padding,
 * restart-marker placement, byte stuffing that spares the markers -- executed on the host with the very code the kernels run.
 * HIPJPEG_STATUS_UNSUPPORTED for baseline output. */
HIPJPEG_API hipjpegStatus_t hipjpegEncodeProgressiveGpuAlgorithmHost(int32_t width, int32_t height, const hipjpegEncodeParams_t* params,
                                                                     const int16_t* const coef[3], uint8_t* out, size_t capacity,
                                                                     size_t* length);
/* The GPU entropy coder's baseline algorithm (csrc/huffman_encode_core.h: per-block coding, the segmented scan of the bit offsets,
 * padding, restart-marker placement, byte stuffing that spares the markers) executed on the host with the very code the kernels run.
 * Any restart_interval (0..65535, 0 = none), Annex-K or optimized tables.  Same signature and output as
 * hipjpegEncodeFromCoefficientsHost; HIPJPEG_STATUS_UNSUPPORTED for progressive output. */
HIPJPEG_API hipjpegStatus_t hipjpegEncodeBaselineGpuAlgorithmHost(int32_t width, int32_t height, const hipjpegEncodeParams_t* params,
                                                                  const int16_t* const coef[3], uint8_t* out, size_t capacity, size_t* length);

/* ---- lossless transcode: entropy decode -> coefficient relayout -> entropy coder; no pixel is computed, every coefficient of the source
 *      survives (what jpegtran -optimize / -progressive do).  The output is the JFIF file hipjpegEncodeFromCoefficientsHost writes for the
 *      source's geometry, coefficients and quantization tables: APP0, components 1/2/3, SOF0 or SOF2, libjpeg's dummy blocks where the MCU
 *      grid overhangs the picture.  APPn / COM segments of the source (EXIF, ICC, comments) are copied only with
 *      HIPJPEG_TRANSCODE_COPY_MARKERS (below).  The source's own restart interval is not carried over.
 *      An image is transcodable when it is SOF0 / SOF1 / SOF2 with 8-bit samples; has one component, or three with colour model YCbCr (RGB
 *      streams -- Adobe transform 0 or component ids R, G, B -- are refused: the writer would label them YCbCr); chroma sampled 1x1 and
 *      luma 1x1, 2x1, 2x2, 1x2, 4x1 or 4x2; every quantizer entry <= 255 and Cb, Cr tables of equal contents; every DC value in
 *      [-1024, 1023] and every AC value in [-1023, 1023] (jchuff.c's limits for 8-bit data).  Anything else is
 *      HIPJPEG_STATUS_UNSUPPORTED; damaged sources keep the decoder's statuses (BAD_JPEG, TRUNCATED, CORRUPT).
 *
 *      Lossless turns (jpegtran -flip / -transpose / -transverse / -rotate): `orientation` 1..8 has the meaning it has in
 *      hipjpegTransform_t -- the output is the source brought upright for that EXIF value (2 horizontal mirror, 3 rotate 180, 4 vertical
 *      mirror, 5 transpose, 6 rotate 90 clockwise, 7 transverse, 8 rotate 270 clockwise).  Orientation 1, the picture as it is, is
 *      written 0 in the field: a 1 there stays HIPJPEG_STATUS_INVALID_ARGUMENT, as it was while the field was reserved.  Blocks change
 *      places, a transposing turn transposes every block, swaps width and height and the luma factors (2x1 <-> 1x2) and transposes the
 *      quantization tables; a mirror negates the coefficients of odd horizontal (vertical) frequency.  No coefficient is requantized.
 *      A mirror moves whole iMCUs only.  In source terms orientations 2, 3, 7, 8 mirror the x axis and 3, 4, 6, 7 the y axis; 5 mirrors
 *      neither.  By default the source's size along every mirrored axis must be a multiple of its iMCU size there (8 * luma factor; 8 for
 *      one component), otherwise the image is HIPJPEG_STATUS_UNSUPPORTED (jpegtran -perfect).  With HIPJPEG_TRANSCODE_TRIM the source is
 *      first cut to whole iMCUs along the mirrored axes, keeping its left / top part, and the output has the cut picture's size (jpegtran
 *      -trim); a mirrored axis shorter than one iMCU is UNSUPPORTED (jpegtran would leave that strip where it is, unmirrored: a file
 *      that is not the turned picture).  Along an axis that is not mirrored ragged edge blocks travel as they are.  Transposing turns of
 *      4x1 or 4x2 luma are UNSUPPORTED (the writer has no 1x4 / 2x4).  The range rule is checked on the blocks that are carried over.
 *      HIPJPEG_TRANSCODE_ORIENTATION_FROM_EXIF takes the orientation from the source's own EXIF tag (hipjpegGetExifOrientation) instead
 *      of the low bits, which must then be 0; without HIPJPEG_TRANSCODE_COPY_MARKERS the output carries no EXIF, so it is upright and says
 *      nothing to the contrary.
 *
 *      Three more operations, applied in this order BEFORE the turn: drop chroma -> crop -> turn.  Each rule speaks of the picture being
 *      written at that step.
 *      HIPJPEG_TRANSCODE_GRAYSCALE (jpegtran -grayscale): a three-component YCbCr source becomes a one-component picture: the luma
 *      component's blocks over ceil(w/8) x ceil(h/8) and the luma table, written 1x1.  The rules that concern chroma only are waived (equal
 *      Cb/Cr tables, chroma quantizers <= 255, chroma sampled 1x1, the list of luma factors, the range rule on chroma blocks); what remains:
 *      SOF0/1/2 with 8-bit samples, one component or three with colour model YCbCr, luma quantizers in 1..255, the range rule on the luma
 *      blocks carried over, and the luma component sampled at the frame's full resolution (its factors are the frame's largest).  On a
 *      one-component source the flag does nothing.  From here on the iMCU is 8x8 (transupp.c: the iMCU of the output's component count).
 *      Crop (jpegtran -crop): a region per image (hipjpegTranscodeRegion_t: stored-image coordinates, end exclusive, all zeros = the whole
 *      picture, as in hipjpegTransform_t).  A region that is not all zeros must satisfy 0 <= x0 < x1 <= width and 0 <= y0 < y1 <= height of
 *      a source that is transcodable at all, else that image is HIPJPEG_STATUS_INVALID_ARGUMENT.  x0 and y0 must be multiples of the iMCU
 *      (8 * luma factors; 8x8 for one component, so also after GRAYSCALE), else HIPJPEG_STATUS_UNSUPPORTED -- unless
 *      HIPJPEG_TRANSCODE_CROP_EXPAND moves the origin left / up to the iMCU boundary; x1 and y1 stay, so the region grows (what jpegtran
 *      -crop does).  The output is (x1 - x0') x (y1 - y0'); every component carries the blocks of its real area for that size, read from
 *      block origin (x0'/8 * h_c/hs, y0'/8 * v_c/vs) of the source's grid.  x1 and y1 need no alignment: a partial edge block travels whole,
 *      and beyond the real area the writer makes libjpeg's dummy blocks.  The range rule is checked on the blocks carried over.  A region
 *      that covers the whole picture writes the file that no region writes.  The turn then applies to the cropped picture: the perfect /
 *      TRIM rule is judged on the cropped size, and trim keeps the cropped picture's left / top part.
 *      HIPJPEG_TRANSCODE_COPY_MARKERS (jpegtran -copy all): every APP0..APP15 and COM segment of the source between SOI and the first SOS
 *      is copied verbatim, in source order, right behind the writer's own JFIF APP0 and before the first DQT.  An APP0 whose payload begins
 *      "JFIF\0" is not copied (the writer has written its own; a JFXX APP0 is); fill bytes in front of markers are not copied; there is no
 *      cap on the total.  When the effective turn is not the identity and the first APP1/Exif segment (the one hipjpegGetExifOrientation
 *      reads) is among the copies, the two value bytes of its orientation tag are overwritten with 1 in the segment's byte order, so the
 *      turned file does not go on asking to be turned.  Nothing else in that segment changes: pixel-dimension tags (PixelXDimension,
 *      ImageWidth, ...) and embedded thumbnails stay as they are, also after a crop. ---- */
#define HIPJPEG_TRANSCODE_ORIENTATION_FROM_EXIF 0x10000 /* or-ed into hipjpegTranscodeParams_t::orientation */
#define HIPJPEG_TRANSCODE_TRIM 0x20000                  /* or-ed into hipjpegTranscodeParams_t::orientation */
#define HIPJPEG_TRANSCODE_GRAYSCALE 0x80000             /* or-ed into hipjpegTranscodeParams_t::orientation */
#define HIPJPEG_TRANSCODE_CROP_EXPAND 0x100000          /* or-ed into hipjpegTranscodeParams_t::orientation */
#define HIPJPEG_TRANSCODE_COPY_MARKERS 0x200000         /* or-ed into hipjpegTranscodeParams_t::orientation */
typedef struct {
    int32_t optimized_huffman; /* as hipjpegEncodeParams_t */
    int32_t progressive;       /* as hipjpegEncodeParams_t */
    int32_t restart_interval;  /* MCUs, 0 = none (the source's own interval is not carried over) */
    int32_t orientation;       /* 0 (none) or 2..8, optionally or-ed with the HIPJPEG_TRANSCODE_* flags above; any other bit is
                                  HIPJPEG_STATUS_INVALID_ARGUMENT */
} hipjpegTranscodeParams_t;
typedef struct {
    int32_t x0, y0, x1, y1; /* stored-image coordinates, end exclusive; all zeros = the whole picture */
} hipjpegTranscodeRegion_t;

/* Host only: the EXIF orientation (tag 0x0112 of IFD0 in the first APP1/Exif segment before the first scan) of a JPEG file, 1..8;
 * 1 when there is no such tag or its value is outside 1..8. */
HIPJPEG_API hipjpegStatus_t hipjpegGetExifOrientation(const uint8_t* data, size_t length, int32_t* orientation);
/* Host only, usable without a GPU: host entropy decoder -> host coder.  HIPJPEG_STATUS_BUFFER_TOO_SMALL with *out_length = needed size
 * if capacity is insufficient (as hipjpegEncodeFromCoefficientsHost). */
HIPJPEG_API hipjpegStatus_t hipjpegTranscodeHost(const uint8_t* data, size_t length, const hipjpegTranscodeParams_t* params, uint8_t* out,
                                                 size_t capacity, size_t* out_length);
/* hipjpegTranscodeHost with a region (NULL = the whole picture); links without the HIP runtime, like hipjpegTranscodeHost. */
HIPJPEG_API hipjpegStatus_t hipjpegTranscodeHostRegion(const uint8_t* data, size_t length, const hipjpegTranscodeParams_t* params,
                                                       const hipjpegTranscodeRegion_t* region, uint8_t* out, size_t capacity, size_t* out_length);
/* Regions for the NEXT hipjpegTranscodeBatch on this handle: batch_size entries (copied), NULL = none; consumed by that one batch; a count
 * that differs from that batch's size makes it return HIPJPEG_STATUS_INVALID_ARGUMENT. */
HIPJPEG_API hipjpegStatus_t hipjpegTranscodeBatchSetRegions(hipjpegHandle_t handle, const hipjpegTranscodeRegion_t* regions, int batch_size);
/* Device: entropy decode, coef_relayout_kernel (csrc/transcode_kernels.hip: decoder layout -> coder layout, with the range check) and the
 * entropy coder in one blocking call on `stream`; the files are then read with hipjpegEncodeGetBitstream(handle, i, ...), which reports
 * the image's status for an image without a file.  `params`: one per image (turned images, and images cropped at an origin other than (0, 0), go
 * through coef_transform_kernel of the same file, the others through coef_relayout_kernel: one launch each).  `flags`: HIPJPEG_FLAG_GPU_HUFFMAN puts both entropy stages
 * on the device for every image each of them takes (the decode side honours hipjpegSetHybridHuffmanThreshold; progressive output with a
 * restart interval goes to the host coder unless HIPJPEG_FLAG_GPU_PROGRESSIVE_RESTART is set), HIPJPEG_FLAG_GPU_RESTART_INTERVALS and
 * HIPJPEG_FLAG_GPU_PROGRESSIVE_RESTART as in hipjpegEncodeBatchEntropy; 0 = both stages on the
 * host pool.  The bytes do not depend on the flags.  A failing image leaves the rest of the batch alone.  The call occupies a decode page
 * and the encode batch of the handle: it must not overlap a hipjpegDecodeBatchSubmit / hipjpegEncodeBatchSubmit still in flight on the
 * same handle (HIPJPEG_STATUS_INVALID_ARGUMENT). */
HIPJPEG_API hipjpegStatus_t hipjpegTranscodeBatch(hipjpegHandle_t handle, const uint8_t* const* data, const size_t* lengths, int batch_size,
                                                  const hipjpegTranscodeParams_t* params, unsigned flags, hipjpegStatus_t* statuses, void* stream);
/* Of the handle's last transcode batch: images the GPU entropy decoder took, images the GPU entropy coder took, blocks the relayout
 * kernels moved (the real blocks of every image that reached them: those of the picture written -- gray, cropped, trimmed, turned). */
HIPJPEG_API hipjpegStatus_t hipjpegTranscodeBatchStats(hipjpegHandle_t handle, int32_t* gpu_decoded_images, int32_t* gpu_coded_images,
                                                       int32_t* relayout_blocks);

/* ---- coefficient tensors: the quantized DCT coefficients between the two entropy stages, read from a JPEG file and written to one
 *      (libjpeg's jpeg_read_coefficients / jpeg_write_coefficients), on the host or as device memory that never leaves HBM.
 *      Layout (one definition for every call below): a component's coefficients are int16 blocks of 64 values in NATURAL order
 *      (row * 8 + column, libjpeg's JBLOCK), the blocks in raster order over the component's REAL block area: blocks_w[c] =
 *      ceil(samp_w[c] / 8) by blocks_h[c] = ceil(samp_h[c] / 8) -- libjpeg's width_in_blocks / height_in_blocks, not the MCU-padded grid.
 *      Block (by, bx) lies at coef[c] + (by * pitch_blocks[c] + bx) * 64 with pitch_blocks[c] >= blocks_w[c]; what lies between blocks_w
 *      and the pitch is neither read nor written.  The values are the quantized ones as the stream codes them; nothing is dequantized.
 *      Quantization tables are uint16[64] in natural order, one per component.
 *
 *      Reading takes every frame the decoder decodes: SOF0 / SOF1 / SOF2 with 8-bit samples, 1..4 components (CMYK / YCCK included), every
 *      sampling layout, multi-scan sequential streams, restart intervals.  Everything else keeps the status decoding gives it
 *      (UNSUPPORTED, BAD_JPEG, TRUNCATED, CORRUPT).  An image that fails writes nothing into its planes.
 *
 *      Writing takes what the writer writes -- the header rules of the lossless transcode above, judged on the `info`: one component, or
 *      three with colour model YCbCr; chroma 1x1 and luma 1x1, 2x1, 2x2, 1x2, 4x1 or 4x2; every quantizer in 1..255 and equal Cb / Cr
 *      tables; every DC value in [-1024, 1023] and every AC value in [-1023, 1023] over the real area.  Otherwise the image is
 *      HIPJPEG_STATUS_UNSUPPORTED.  HIPJPEG_STATUS_INVALID_ARGUMENT for that image: a size outside 1..65535, blocks_w / blocks_h that
 *      are not what the geometry gives, a pitch below blocks_w, a null pointer, a pointer that is not 16-byte aligned, a restart
 *      interval outside 0..65535, a `params.orientation` other than 0.  The file is the one hipjpegEncodeFromCoefficientsHost writes for
 *      that geometry, those coefficients and those tables: APP0, components 1/2/3, SOF0 or SOF2, libjpeg's dummy blocks beyond the real
 *      area; no APPn / COM is carried.  Writing what was read from a transcodable source gives, byte for byte, the file
 *      hipjpegTranscodeHost writes for the same coding parameters. ---- */
typedef struct {
    int32_t width, height, num_components; /* 1..4 when read; 1 or 3 when written */
    int32_t color_model;                   /* as hipjpegImageInfo_t */
    int32_t h[4], v[4];
    int32_t blocks_w[4], blocks_h[4];      /* real block area per component */
    uint16_t qtable[4][64];                /* natural order */
} hipjpegCoefficientInfo_t;

typedef struct {
    void* coef[4]; /* device (or host, for the *Host calls) int16, 16-byte aligned */
    uint32_t pitch_blocks[4];
} hipjpegCoefficientPlanes_t;

/* Host only: geometry and tables from the header, so that a caller can allocate before decoding. */
HIPJPEG_API hipjpegStatus_t hipjpegGetCoefficientInfo(const uint8_t* data, size_t length, hipjpegCoefficientInfo_t* info);
/* Host only, usable without a GPU (links without the HIP runtime, like hipjpegTranscodeHost): host entropy decoder -> planes. */
HIPJPEG_API hipjpegStatus_t hipjpegDecodeCoefficientsHost(const uint8_t* data, size_t length, const hipjpegCoefficientPlanes_t* planes);
/* Host only: planes -> host coder.  `params`: optimized_huffman, progressive, restart_interval; orientation must be 0.
 * HIPJPEG_STATUS_BUFFER_TOO_SMALL with *out_length = needed size if capacity is insufficient (as hipjpegEncodeFromCoefficientsHost). */
HIPJPEG_API hipjpegStatus_t hipjpegEncodeCoefficientsHost(const hipjpegCoefficientInfo_t* info, const hipjpegCoefficientPlanes_t* planes,
                                                          const hipjpegTranscodeParams_t* params, uint8_t* out, size_t capacity,
                                                          size_t* out_length);
/* Device: entropy decode (`flags` as in hipjpegTranscodeBatch: HIPJPEG_FLAG_GPU_HUFFMAN = on the device for every image it takes,
 * honouring hipjpegSetHybridHuffmanThreshold; 0 = host pool), then coef_export_kernel (csrc/coefficient_kernels.hip: decoder layout ->
 * planes[i]) queued on `stream`.  The call returns with final statuses -- the entropy verdicts are settled -- and the caller orders on
 * `stream` before reading the planes.  The tensors do not depend on the flags.  A failing image leaves its planes and the rest of the
 * batch alone.  The call takes the handle's current decode page: it must not overlap a hipjpegDecodeBatchSubmit /
 * hipjpegEncodeBatchSubmit still in flight on the same handle (HIPJPEG_STATUS_INVALID_ARGUMENT). */
HIPJPEG_API hipjpegStatus_t hipjpegDecodeCoefficientsBatch(hipjpegHandle_t handle, const uint8_t* const* data, const size_t* lengths, int batch_size,
                                                           const hipjpegCoefficientPlanes_t* planes, unsigned flags, hipjpegStatus_t* statuses,
                                                           void* stream);
/* Device: coef_import_kernel (planes[i] -> the coder's layout, with the range check) queued on `stream` -- planes produced on that
 * stream need no extra synchronisation -- then the entropy coder (`flags` as in hipjpegTranscodeBatch); blocks until the files exist.
 * They are then read with hipjpegEncodeGetBitstream(handle, i, ...), which reports the image's status for an image without a file.  The
 * bytes do not depend on the flags.  The call takes the handle's encode batch: the same rule about Submits in flight. */
HIPJPEG_API hipjpegStatus_t hipjpegEncodeCoefficientsBatch(hipjpegHandle_t handle, const hipjpegCoefficientInfo_t* infos,
                                                           const hipjpegCoefficientPlanes_t* planes, const hipjpegTranscodeParams_t* params,
                                                           int batch_size, unsigned flags, hipjpegStatus_t* statuses, void* stream);
/* Coefficient tensors to pixels: coef_to_decoder_kernel (csrc/coefficient_kernels.hip: planes[i] -> the decoder's layout) and then the
 * pixel kernels of hipjpegDecodeBatch (dequantize, IDCT, upsampling, colour, geometry), all queued on `stream` -- planes produced on that
 * stream need no extra synchronisation, no coefficient crosses PCIe, there is no entropy stage.  `infos` / `planes` as in
 * hipjpegEncodeCoefficientsBatch, `outputs` / `format` as in hipjpegDecodeBatch; of `flags`, HIPJPEG_FLAG_FANCY_UPSAMPLING and
 * HIPJPEG_FLAG_FAST_IDCT mean what they mean there and HIPJPEG_FLAG_GPU_HUFFMAN is ignored.  Transforms set with
 * hipjpegDecodeBatchSetTransforms apply to this batch and are consumed by it.
 * For an image whose planes and tables are what hipjpegDecodeCoefficientsHost / hipjpegGetCoefficientInfo give for a file, the output is
 * bit for bit what hipjpegDecodeBatch writes for that file with the same format and flags.  No range rule applies: any int16 is a
 * coefficient and gets the decoder's arithmetic (the SIMD routines' 16-bit wrapping); the quantizers are taken as given, as the parser
 * takes them from a DQT.  Taken: one component, or three with color_model 0 / 1 / 2 as the decoder treats a file of that colour model;
 * every sampling layout and every output format the decoder takes for such a file (HIPJPEG_OUTPUT_YUV_PLANAR under its own rules).
 * HIPJPEG_STATUS_UNSUPPORTED for FOUR components: the CMYK -> RGB formula turns on whether the file carried an Adobe APP14 segment, and
 * hipjpegCoefficientInfo_t does not say.  HIPJPEG_STATUS_INVALID_ARGUMENT for that image: a size outside 1..65535, sampling factors
 * outside 1..4, blocks_w / blocks_h that are not what the geometry gives, a pitch below blocks_w, a null pointer, a pointer that is not
 * 16-byte aligned, an output the pitch and pointer rules of hipjpegDecodeBatch refuse.  A failing image writes nothing to its output and
 * leaves the rest of the batch alone.
 * The call returns when the last kernel is queued; `statuses` are final at return (only argument and header rules can fail).  It takes
 * the handle's current decode page: the rule about Submits in flight of hipjpegDecodeCoefficientsBatch. */
HIPJPEG_API hipjpegStatus_t hipjpegCoefficientsToPixelsBatch(hipjpegHandle_t handle, const hipjpegCoefficientInfo_t* infos,
                                                             const hipjpegCoefficientPlanes_t* planes, int batch_size, const hipjpegOutput_t* outputs,
                                                             hipjpegOutputFormat_t format, unsigned flags, hipjpegStatus_t* statuses, void* stream);
/* Host only, usable without a GPU: the `info` of the file hipjpegEncodeBatch writes for a width x height picture and `params` --
 * components and sampling factors of params->subsampling, colour model gray or YCbCr, real block areas, the quality-scaled Annex-K
 * tables in natural order -- so that a caller can allocate for hipjpegPixelsToCoefficientsBatch.  Only `quality` and `subsampling` are
 * read.  HIPJPEG_STATUS_UNSUPPORTED for an unknown subsampling, HIPJPEG_STATUS_INVALID_ARGUMENT for a size outside 1..65535. */
HIPJPEG_API hipjpegStatus_t hipjpegGetEncodeCoefficientInfo(int32_t width, int32_t height, const hipjpegEncodeParams_t* params,
                                                            hipjpegCoefficientInfo_t* info);
/* Pixels to coefficient tensors: the forward kernels of hipjpegEncodeBatchDevice (colour conversion, downsampling, FDCT, quantization) and
 * then coef_from_coder_kernel (csrc/coefficient_kernels.hip: the coder's layout -> planes[i]), all queued on `stream`; nothing is entropy
 * coded and nothing blocks.  `inputs` / `params` as in hipjpegEncodeBatchDevice (every input format, every subsampling), `planes` as in
 * hipjpegDecodeCoefficientsBatch.  For every image the planes get what hipjpegDecodeCoefficientsHost reads from the file hipjpegEncodeBatch
 * writes for the same pixels and parameters, over the real block area of hipjpegGetEncodeCoefficientInfo; nothing between blocks_w and
 * the pitch is written.  restart_interval, optimized_huffman and progressive do not change coefficients and are ignored beyond the
 * argument rules.  Statuses: those of hipjpegEncodeBatchDevice, then the rules for planes (a pitch below blocks_w, a null pointer, a
 * pointer that is not 16-byte aligned: HIPJPEG_STATUS_INVALID_ARGUMENT); final at return.  A failing image writes nothing into its
 * planes.  The call takes the handle's encode batch: the same rule about Submits in flight. */
HIPJPEG_API hipjpegStatus_t hipjpegPixelsToCoefficientsBatch(hipjpegHandle_t handle, const hipjpegEncodeInput_t* inputs,
                                                             const hipjpegEncodeParams_t* params, int batch_size,
                                                             const hipjpegCoefficientPlanes_t* planes, hipjpegStatus_t* statuses, void* stream);
/* Of the handle's last hipjpegDecodeCoefficientsBatch: images the GPU entropy decoder took; of its last hipjpegEncodeCoefficientsBatch:
 * images the GPU entropy coder took; and the blocks the last of the four calls (those two, hipjpegCoefficientsToPixelsBatch,
 * hipjpegPixelsToCoefficientsBatch) moved (the real blocks of every image that reached its kernel). */
HIPJPEG_API hipjpegStatus_t hipjpegCoefficientsBatchStats(hipjpegHandle_t handle, int32_t* gpu_decoded_images, int32_t* gpu_coded_images,
                                                          int64_t* moved_blocks);

/* ---------------------------------------------------------------- lossless JPEG (SOF3, Huffman): decoding
 * Entry points of their own: every call above still answers HIPJPEG_STATUS_UNSUPPORTED for a lossless frame.  A frame is taken when
 * its precision is 2..16, it has 1..4 components that all have h = v = 1, one scan holds them all, Ss (the predictor) is 1..7,
 * Se = Ah = 0, Al (the point transform) < precision, every table the scan names is there and has no symbol above 16, and the
 * restart interval is 0 or a multiple of the width.  A valid file outside these rules (subsampled components, a scan per component, a
 * restart interval that is not whole rows) is UNSUPPORTED, a malformed one BAD_JPEG.
 * The samples come out as stored: no colour conversion, no clamp.  A sample is the low 16 bits of state << Al, or its low 8 bits when
 * precision <= 8 (libjpeg-turbo's jdlossls.c gives exactly these values). */
typedef struct {
    int32_t width, height, num_components;
    int32_t precision;        /* 2..16 */
    int32_t predictor;        /* Ss: 1..7 */
    int32_t point_transform;  /* Al */
    int32_t restart_rows;     /* rows per restart interval, 0 = none */
    int32_t component_id[4];
} hipjpegLosslessInfo_t;

typedef struct {
    void* plane[4];        /* planar: one pointer per component; interleaved: plane[0] only */
    uint32_t pitch[4];     /* bytes per row; any value that holds a row, any alignment */
    int32_t sample_bytes;  /* 2: uint16 samples; 1: uint8 samples, for precision <= 8 only (else the image is UNSUPPORTED) */
    int32_t planar;        /* 0: H x W x N interleaved; 1: N planes of H x W */
} hipjpegLosslessOutput_t;

/* The reconstruction kernels' shape, for tests that place pictures on their seams: rows of a band and columns of an LDS tile of
 * lossless_wavefront_kernel (predictors 2..7, one wave per component), samples of a row chunk of lossless_rows_kernel (predictor 1,
 * one workgroup per row, a carried sum from chunk to chunk), and the width below which predictor 1 takes the wavefront kernel too. */
typedef struct {
    int32_t band_rows, tile_columns, chunk_samples, rows_min_width;
} hipjpegLosslessKernelShape_t;
HIPJPEG_API hipjpegStatus_t hipjpegLosslessKernelShape(hipjpegLosslessKernelShape_t* shape);

HIPJPEG_API hipjpegStatus_t hipjpegGetLosslessInfo(const uint8_t* data, size_t length, hipjpegLosslessInfo_t* info);
/* Entropy stage and reconstruction on the CPU, into host memory. */
HIPJPEG_API hipjpegStatus_t hipjpegDecodeLosslessHost(const uint8_t* data, size_t length, const hipjpegLosslessOutput_t* output);
/* The same result by the kernels' own schedule run on the host, lane by lane (bands, skew and tiles; column sums, chunks and carried
 * sums).  kernel: 0 = the one the planner picks for this picture, 1 = lossless_rows_kernel (predictor 1 only, else INVALID_ARGUMENT),
 * 2 = lossless_wavefront_kernel. */
HIPJPEG_API hipjpegStatus_t hipjpegLosslessReconstructAlgorithmHost(const uint8_t* data, size_t length, const hipjpegLosslessOutput_t* output,
                                                                    int kernel);
/* Decodes a batch into device memory, asynchronously on `stream`: the entropy stage runs on the handle's host threads, the
 * differences travel in one copy, the reconstruction kernels write the caller's layout.  statuses[i] is final on return; a failing
 * image leaves its output untouched and does not disturb the others.  The outputs may be used once `stream` has reached this point. */
HIPJPEG_API hipjpegStatus_t hipjpegDecodeLosslessBatch(hipjpegHandle_t handle, const uint8_t* const* data, const size_t* lengths, int batch_size,
                                                       const hipjpegLosslessOutput_t* outputs, hipjpegStatus_t* statuses, void* stream);
/* Measurement aid, like hipjpegDecodeBatchDeviceKernel: queues one part of the handle's last hipjpegDecodeLosslessBatch again on `stream`
 * (which: 0 = the host-to-device copy, 1 = the column sums and lossless_rows_kernel, 2 = lossless_wavefront_kernel).  The outputs of
 * that batch must still exist; they are rewritten with the same samples. */
HIPJPEG_API hipjpegStatus_t hipjpegDecodeLosslessBatchDeviceKernel(hipjpegHandle_t handle, int which, void* stream);
/* Of the handle's last hipjpegDecodeLosslessBatch: images through lossless_rows_kernel, images through lossless_wavefront_kernel,
 * bytes of the host-to-device copy. */
HIPJPEG_API hipjpegStatus_t hipjpegDecodeLosslessBatchStats(hipjpegHandle_t handle, int32_t images_per_kernel[2], uint64_t* h2d_bytes);

/* ---- the same with the entropy stage on the GPU, opt-in.  hipjpegDecodeLosslessBatch is flags = 0.
 * HIPJPEG_FLAG_GPU_HUFFMAN sends every frame the lossless decoder takes through GPU kernels that remove the byte stuffing, find the
 * samples of the scan with a self-synchronising walk (one lane per subsequence of the destuffed stream, restart intervals apart) and
 * write the difference planes the host stage would have uploaded: only the compressed scans travel to the device.
 * The contract is that of hipjpegDecodeLosslessBatch: statuses[i] is final on return, a failing image leaves its output untouched and
 * does not disturb the others.  To keep it the call WAITS ONCE per batch, on `stream`, for the verdict words of the entropy kernels,
 * before any reconstruction kernel is queued.  An image whose walk did not converge within the round budget, or that the device
 * flagged (a code no table holds, a scan that ends inside a sample, an interval with too many or too few samples), is decoded again by
 * the host stage, which yields its exact status and, if it succeeds, its differences; those are then uploaded.  The host stage also
 * takes, from the start, an image whose restart markers are not RST0..7 in turn, one with an empty interval, one with a table of
 * more than 32 symbols, and one whose scan is 2^29 bytes or longer: bit positions and sample counts are 32-bit in the kernels, and
 * the bound is taken on the stuffed bytes, so no destuffed scan of 2^32 bits or more reaches them.  Other flags are ignored. */
HIPJPEG_API hipjpegStatus_t hipjpegDecodeLosslessBatchFlags(hipjpegHandle_t handle, const uint8_t* const* data, const size_t* lengths, int batch_size,
                                                            const hipjpegLosslessOutput_t* outputs, hipjpegStatus_t* statuses, unsigned int flags,
                                                            void* stream);
/* hipjpegDecodeLosslessBatchDeviceKernel also takes which = 3 (destuffing, pass 0 and the ripple launches of the GPU entropy stage) and
 * which = 4 (its write pass) behind a call with HIPJPEG_FLAG_GPU_HUFFMAN in which no image went to the host stage (else
 * INVALID_ARGUMENT: the write pass would store over the differences the host stage uploaded). */
/* Of the handle's last lossless batch call: images whose differences the entropy kernels made, images the host stage decoded although
 * the flag was set, ripple launches in which a workgroup had a correction to carry.  All 0 behind a call without the flag. */
HIPJPEG_API hipjpegStatus_t hipjpegDecodeLosslessBatchEntropyStats(hipjpegHandle_t handle, int32_t* gpu_images, int32_t* host_fallback_images,
                                                                   int32_t* ripple_launches);
/* The entropy kernels' shape, for tests that steer streams onto their seams: bits of a subsequence (one lane's share of a destuffed
 * interval), subsequences of a workgroup, correction rounds a workgroup runs per launch, and launches behind the first that carry
 * corrections across workgroup borders. */
typedef struct {
    int32_t subsequence_bits, subsequences_per_workgroup, max_rounds, max_ripple_launches;
} hipjpegLosslessEntropyShape_t;
HIPJPEG_API hipjpegStatus_t hipjpegLosslessEntropyShape(hipjpegLosslessEntropyShape_t* shape);
/* The entropy kernels' schedule run on the CPU, lane by lane: destuffing, pass 0, rounds, ripple launches, checks, sums and stores.
 * Needs no GPU.  planes[c]: differences of frame component c, `pitch` samples (uint16) per row, pitch >= width.  *converged = 0: the
 * rounds did not converge within the budget.  Like the batch call, it then -- and when the walk flagged the image or the marker scan
 * turned it away -- lets the host stage decode, and returns that stage's status and differences. */
HIPJPEG_API hipjpegStatus_t hipjpegLosslessEntropyAlgorithmHost(const uint8_t* data, size_t length, uint16_t* const planes[4], size_t pitch,
                                                                int32_t* converged);
/* The plugin decoder's lossless route (option hipjpeg_decoder:gpu_lossless_entropy=1 sets the flag there): images whose differences
 * the entropy kernels made and images the host stage decoded although the option was set, summed over every decode call of every
 * plugin decoder of this process.  Both stay as they are while the option is off. */
HIPJPEG_API hipjpegStatus_t hipjpegPluginLosslessEntropyStats(int64_t* gpu_images, int64_t* host_fallback_images);
/* The host entropy stage alone (what hipjpegDecodeLosslessBatch runs on its threads): the same planes, for comparison. */
HIPJPEG_API hipjpegStatus_t hipjpegLosslessEntropyHost(const uint8_t* data, size_t length, uint16_t* const planes[4], size_t pitch);

/* ---------------------------------------------------------------- lossless JPEG (SOF3, Huffman): encoding
 * Byte for byte the file libjpeg-turbo writes in lossless mode (jpeg_enable_lossless; jclossls.c / jclhuff.c) from the same samples:
 * state x = sample >> point_transform, predicted from the states to the left, above and above-left of the INPUT with the decoder's
 * rules (first sample of the picture and of every restart interval 1 << (P - Pt - 1), rest of that row from the left, column 0 from
 * above, elsewhere the predictor), difference = (x - prediction) & 0xFFFF, category SSSS 0..16 (16 = 32768, no extra bits).  One scan
 * holds all components sample by sample.  The library forces optimized coding in lossless mode: every file carries ONE table, built
 * from the category counts of all its components together (jpeg_gen_optimal_table), which every component names (Td = 0).  Segment
 * order: SOI, APPn, SOF3, DHT, [DRI = restart_rows * width], SOS, scan, EOI.  One component: JFIF APP0, id 1; three: Adobe APP14 with
 * transform 0, ids 'R' 'G' 'B'; four: Adobe APP14, ids 'C' 'M' 'Y' 'K'; two: no APPn, ids 0, 1.  A restart interval is a whole
 * number of rows.  Samples above 2^P - 1 are the caller's error: the file is then unspecified, the call still memory-safe.
 * INVALID_ARGUMENT: precision outside 2..16, predictor outside 1..7, point_transform >= precision (or negative), num_components outside
 * 1..4, restart_rows negative, a width or height outside 1..65535, restart_rows * width above 65535 (DRI is 16 bits), sample_bytes other
 * than 1 or 2, sample_bytes == 1 with precision > 8, a missing plane, or a pitch shorter than a row. */
typedef struct {
    int32_t precision;        /* P: 2..16 */
    int32_t predictor;        /* Ps: 1..7 */
    int32_t point_transform;  /* Pt: 0 .. P - 1 */
    int32_t restart_rows;     /* rows per restart interval, 0 = none */
    int32_t num_components;   /* 1..4 */
} hipjpegLosslessEncodeParams_t;

/* The const twin of hipjpegLosslessOutput_t, with the picture's size */
typedef struct {
    const void* plane[4];  /* planar: one pointer per component; interleaved: plane[0] only */
    uint32_t pitch[4];     /* bytes per row; any value that holds a row, any alignment */
    int32_t sample_bytes;  /* 2: uint16 samples; 1: uint8 samples, for precision <= 8 only */
    int32_t planar;        /* 0: H x W x N interleaved; 1: N planes of H x W */
    int32_t width, height;
} hipjpegLosslessEncodeInput_t;

/* The coder kernels' shape, for tests that aim at their seams: samples of a group (one lane codes a group of consecutive samples of
 * the scan, whatever rows and restart intervals end inside it), samples of a workgroup of the length / write kernels (the write
 * kernel's LDS window), bytes of a stuffing chunk (count / expand kernels). */
typedef struct {
    int32_t group_samples, window_samples, chunk_bytes;
} hipjpegLosslessEncodeShape_t;
HIPJPEG_API hipjpegStatus_t hipjpegLosslessEncodeShape(hipjpegLosslessEncodeShape_t* shape);
/* The kernels' bit offsets are uint32: a picture is taken when 31 * samples + 24 * intervals <= 2^32 - 1 (samples = width * height *
 * components; intervals = restart intervals of the scan, 1 without).  Returns 1 when it fits, 0 when the batch call answers
 * HIPJPEG_STATUS_UNSUPPORTED for it.  Host only. */
HIPJPEG_API int hipjpegLosslessEncodeFitsGpu(uint64_t samples, uint64_t intervals);

/* Host samples in, file out, coded sample by sample as the library does it.  Needs no GPU.  HIPJPEG_STATUS_BUFFER_TOO_SMALL with
 * *out_length = needed size if capacity is insufficient (as hipjpegEncodeFromCoefficientsHost). */
HIPJPEG_API hipjpegStatus_t hipjpegEncodeLosslessHost(const hipjpegLosslessEncodeInput_t* input, const hipjpegLosslessEncodeParams_t* params,
                                                      uint8_t* out, size_t capacity, size_t* out_length);
/* The same file by the kernels' schedule run on the host, lane by lane: groups, per-workgroup counters, the segmented scan over the
 * lanes' ranges, LDS windows with shared end words, marker bitmap, stuffing chunk by chunk.  Needs no GPU. */
HIPJPEG_API hipjpegStatus_t hipjpegEncodeLosslessGpuAlgorithmHost(const hipjpegLosslessEncodeInput_t* input,
                                                                  const hipjpegLosslessEncodeParams_t* params, uint8_t* out, size_t capacity,
                                                                  size_t* out_length);
/* Codes a batch of pictures that lie in device memory, on `stream`: statistics, lengths, offsets, bits, stuffing and file assembly all
 * run in kernels; the category counts and the total bits come to the host (the call waits for each, twice per batch), the files land
 * in pinned host memory.  statuses[i] is final on return; an image with bad parameters gets its status and does not disturb the
 * others; UNSUPPORTED where hipjpegLosslessEncodeFitsGpu says 0.  There is no host fallback inside the call.  The inputs may be
 * released once `stream` has reached this point; hipjpegEncodeLosslessGetBitstream waits for that itself. */
HIPJPEG_API hipjpegStatus_t hipjpegEncodeLosslessBatch(hipjpegHandle_t handle, const hipjpegLosslessEncodeInput_t* inputs,
                                                       const hipjpegLosslessEncodeParams_t* params, int batch_size, hipjpegStatus_t* statuses,
                                                       void* stream);
/* File `index` of the handle's last hipjpegEncodeLosslessBatch: valid until the third batch behind it (three pages are used in turn).
 * INVALID_ARGUMENT for an image that failed. */
HIPJPEG_API hipjpegStatus_t hipjpegEncodeLosslessGetBitstream(hipjpegHandle_t handle, int index, const uint8_t** data, size_t* length);
/* Of the handle's last hipjpegEncodeLosslessBatch: images the kernels coded, times the call waited for the device, bytes of the bit
 * buffers (marker bitmaps included). */
HIPJPEG_API hipjpegStatus_t hipjpegEncodeLosslessBatchStats(hipjpegHandle_t handle, int32_t* gpu_images, int32_t* waits, uint64_t* bit_buffer_bytes);
/* Measurement aid: the stages of the handle's last hipjpegEncodeLosslessBatch by HIP events on its stream, in milliseconds (waits for the
 * batch's end): 0 descriptors up + lenc_stats_kernel, 1 counts down, the first wait and the host's tables, 2 codes up + lenc_length_kernel,
 * 3 lenc_scan_kernel, 4 totals down, the second wait and the host's layout, 5 descriptors up + clearing the bit buffers,
 * 6 lenc_write_kernel, 7 count + layout, 8 expand (the files, into pinned memory when it is the library's), 9 the copies behind it. */
HIPJPEG_API hipjpegStatus_t hipjpegEncodeLosslessBatchStageTimes(hipjpegHandle_t handle, float milliseconds[10]);

#ifdef __cplusplus
}
#endif
#endif /* HIPJPEG_H_ */
