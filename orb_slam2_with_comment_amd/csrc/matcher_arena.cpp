// The matcher handle's staging arena (matcher.h): device blocks with pinned host mirrors, in
// generations, and the merged upload range.  Used through capi_stage.h's call scope.
#include <algorithm>
#include <cstring>

#include "matcher.h"

namespace orbmi {

void* Matcher::stage(size_t bytes) {
    bytes = (bytes + 255) & ~(size_t)255;
    std::vector<Block>& arena = gens[gen].blocks;
    for (Block& b : arena)
        if (b.size - b.used >= bytes) { void* p = b.p + b.used; b.used += bytes; return p; }
    Block b{nullptr, std::max(bytes, (size_t)(4 << 20)), 0, nullptr};
    if (hipMalloc((void**)&b.p, b.size) != hipSuccess) return nullptr;
    if (hipHostMalloc((void**)&b.h, b.size, hipHostMallocDefault) != hipSuccess) {
        (void)hipFree(b.p);
        return nullptr;
    }
    b.used = bytes;
    arena.push_back(b);
    return b.p;
}

uint8_t* Matcher::mirror(const void* d) {
    const uint8_t* q = (const uint8_t*)d;
    for (Block& b : gens[gen].blocks)
        if (q >= b.p && q < b.p + b.size) return b.h + (q - b.p);
    return nullptr;
}

hipError_t Matcher::flush_up() {
    if (!up.n) return hipSuccess;
    const hipError_t e = hipMemcpyAsync(up.d, up.h, up.n, hipMemcpyHostToDevice, stream);
    up.n = 0;
    if (e != hipSuccess && up_err == hipSuccess) up_err = e;
    return e;
}

hipError_t Matcher::h2d(void* d, const void* src, size_t bytes) {
    if (!bytes) return hipSuccess;
    uint8_t* h = mirror(d);
    if (!h) return hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, ls());
    memcpy(h, src, bytes);
    // the allocation right after the pending range (stage() rounds to 256 B; the gap is the
    // previous allocation's padding): extend the range, else send it and start a new one
    const size_t end = (up.n + 255) & ~(size_t)255;
    if (up.n && (uint8_t*)d == up.d + end && h == up.h + end) {
        up.n = end + bytes;
        return hipSuccess;
    }
    const hipError_t e = flush_up();
    up = PendUp{(uint8_t*)d, h, bytes};
    return e;
}

hipError_t Matcher::d2h(void* user, const void* d, size_t bytes) {
    if (!bytes) return hipSuccess;
    uint8_t* h = mirror(d);
    if (!h) return hipMemcpyAsync(user, d, bytes, hipMemcpyDeviceToHost, ls());
    pend.push_back(Pend{user, h, bytes});
    return hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, ls());
}

void Matcher::d2h_flush() {
    for (const Pend& p : pend) memcpy(p.user, p.mirror, p.bytes);
    pend.clear();
}

void Matcher::arena_reset() {
    // (a finished call leaves nothing pending, and the call scope of one that failed drops what
    // it staged; kept for safety)
    (void)flush_up();
    up_err = hipSuccess;
    // the generation just used may still be read by the work enqueued so far: mark it with an
    // event, move on, and wait only for the generation about to be reused
    bool used = false;
    for (Block& b : gens[gen].blocks) used |= b.used > 0;
    if (used) {
        if (!gens[gen].ev && hipEventCreateWithFlags(&gens[gen].ev, hipEventDisableTiming) != hipSuccess) {
            gens[gen].ev = nullptr;
            (void)hipStreamSynchronize(stream);  // no event: fall back to a full wait
        } else if (gens[gen].ev) {
            (void)hipEventRecord(gens[gen].ev, stream);
            gens[gen].pending = true;
        }
        gen = (gen + 1) % kArenaGens;
    }
    Gen& g = gens[gen];
    if (g.pending) {
        (void)hipEventSynchronize(g.ev);
        g.pending = false;
    }
    for (Block& b : g.blocks) b.used = 0;
    pend.clear();
}

void Matcher::release() {
    (void)hipSetDevice(device);
    if (stream) (void)flush_up();
    if (stream) (void)hipStreamSynchronize(stream);  // staged inputs may still be read
    void* ptrs[] = {d_cell_start, d_cell_list, d_kp_cell, d_mcell_start, d_mcell_list, d_mkp_cell, d_cand, d_ncand, d_top,
                    d_res, d_bin_of, d_hist, d_scalars, d_track};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    for (GridSlot& g : gslot) {
        if (g.cs) (void)hipFree(g.cs);
        if (g.cl) (void)hipFree(g.cl);
        if (g.kc) (void)hipFree(g.kc);
        g = GridSlot{};
    }
    for (Gen& g : gens) {
        for (Block& b : g.blocks) {
            (void)hipFree(b.p);
            if (b.h) (void)hipHostFree(b.h);
        }
        g.blocks.clear();
        if (g.ev) (void)hipEventDestroy(g.ev);
        g.ev = nullptr;
        g.pending = false;
    }
    if (stream && own_stream) (void)hipStreamDestroy(stream);
    stream = nullptr;
}

}  // namespace orbmi
