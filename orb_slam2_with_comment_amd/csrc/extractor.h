// The extractor's handle (shared by extractor.hip, stereo.hip, capi_extract.cpp): the tables and the
// plan of the current image size (extractor_plan.h, HIP-free: everything the host computes), their
// device mirrors, and the grow-only device buffers.
#pragma once
#include <array>
#include <vector>

#include "orbmi_common.h"

namespace orbmi {

// Grow-only device buffer.  On failure *p is null and *cap is 0: the next call allocates again.
template <class T>
inline int ensure_buf(T** p, size_t* cap, size_t n) {
    if (*p && *cap >= n) return ORBMI_OK;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    if (n == 0) n = 1;
    ORBMI_HIP(hipMalloc((void**)p, n * sizeof(T)));
    *cap = n;
    return ORBMI_OK;
}

struct Extractor {
    int device = 0;
    int ini_th = 0, min_th = 0;
    OrbTables tab;       // of the constructor's parameters
    // The geometry of the current image size.  rows == cols == 0 and an empty plan: none, and
    // set_geometry plans again; otherwise the device mirrors below hold exactly this plan.
    int rows = 0, cols = 0;
    ExtractorPlan plan;
    int blur_mode = -1;  // GaussianBlur (ORBMI_BLUR): -1 by batch, 0 side stream, 1 in the octree launch, 2 after it
    hipStream_t bstream = nullptr;  // the blur's side stream
    hipEvent_t ev_pyr = nullptr, ev_blur = nullptr;

    // device buffers (capacity for `bcap` images)
    int bcap = 0;
    hipStream_t stream = nullptr;
    LevelGeom* d_levels = nullptr;
    CellGeom* d_cells = nullptr;
    XTab* d_xtab = nullptr;
    YTab* d_ytab = nullptr;
    uint8_t* d_pyr = nullptr;
    uint8_t* d_blur = nullptr;     // blurred levels: interior only, rows of bstride bytes
    int2* d_btiles = nullptr;      // blur tiles: {level, x0 | y0 << 16}
    int* d_level_count = nullptr;   // [b][level][region] FAST candidates (k_fast2 allocates, k_pyr_level0 clears)
    int* d_regbase = nullptr;       // [level][region] first slot of each candidate region (per image)
    uint32_t* d_pyr_blob = nullptr; // k_pyramid parameter blocks, plan.blob_words per tile
    uint2* d_cand = nullptr;        // [b][keys_cap] {x | y << 12 | score << 24, cell << 10 | rank}
    uint32_t* d_node_of = nullptr;  // octree node | depth << 16 of keys beyond the register-resident ones
    uint2* d_oct = nullptr;        // {x | y << 16 (level coords), score}
    int* d_oct_count = nullptr;    // [b][level]
    // last outputs (host API and stereo input)
    int out_capacity = 0;          // keypoints per image in d_kps / d_desc
    orbmi_keypoint* d_kps = nullptr;
    uint8_t* d_desc = nullptr;
    int* d_counts = nullptr;
    uint8_t* d_image = nullptr;    // staging for host images
    size_t image_bytes = 0;
    // pageable host images of orbmi_extract_batch_host: pinned staging, two alternating buffers,
    // each guarded by the event after the copy kernel that reads it
    uint8_t* h_stage[2] = {nullptr, nullptr};
    size_t stage_bytes[2] = {0, 0};
    hipEvent_t stage_ev[2] = {nullptr, nullptr};
    int stage_next = 0;
    int last_batch = 0;
    // last batch output location (may be caller buffers for the device API)
    orbmi_keypoint* last_kps = nullptr;
    uint8_t* last_desc = nullptr;
    int* last_counts = nullptr;
    int last_capacity = 0;
    // stereo scratch
    float* d_scale_tab = nullptr;  // [scale | inv_scale], 2*nlevels floats
    int* d_row_start = nullptr;
    int* d_row_list = nullptr;
    int* d_sad = nullptr;
    size_t row_cap = 0, row_list_cap = 0, sad_cap = 0, stereo_u_cap = 0, stereo_d_cap = 0;
    float* d_stereo_u = nullptr;
    float* d_stereo_d = nullptr;

    // per-stage HIP-event profiling (orbmi_set_profiling / orbmi_read_profile)
    unsigned prof_mask = 0;
    struct ProfPair { int stage; hipEvent_t a, b; };
    std::vector<ProfPair> prof_pending;
    std::vector<hipEvent_t> prof_pool;
    hipEvent_t prof_event();
    hipEvent_t prof_begin(int stage, hipStream_t s = nullptr);
    void prof_end(int stage, hipEvent_t a, hipStream_t s = nullptr);

    struct GeomTable { void** dev; const void* host; size_t bytes; };
    std::array<GeomTable, 7> geom_tables(const ExtractorPlan& p);  // the plan's tables and their device mirrors

    int init(int dev, int nf, float sf, int nl, int ini, int mn);
    int set_geometry(int rows, int cols);
    int reserve(int batch, int capacity);
    int ensure_side_stream();  // bstream + its events on first use (large batches only)
    // host images -> d_image by a copy kernel on `stream` (pinned memory read in place, pageable
    // memory staged first); *d_out = d_image
    int upload_host(const uint8_t* h_images, size_t bytes, const uint8_t** d_out);
    int run(const uint8_t* d_images, int batch, size_t step, size_t image_stride,
            orbmi_keypoint* kps, uint8_t* desc, int* counts, int capacity);
    void release();
};

}  // namespace orbmi
