// Device-resident task lists of the C ABI (host side): shared by api_lists.hip, api_recon.hip, api_intra.hip (lists made from whole task arrays) and chunk.hip
// (lists assembled from per-tile-sbrow chunks that were preprocessed on the submitting threads).
#pragma once
#include "capi.h"
#include <vector>
#include <unordered_map>

#define MC_BINS 15

static const uint8_t k_tx_w[19] = { 4, 8, 16, 32, 64, 4, 8, 8, 16, 16, 32, 32, 64, 4, 16, 8, 32, 16, 64 };
static const uint8_t k_tx_h[19] = { 4, 8, 16, 32, 64, 8, 4, 16, 8, 32, 16, 64, 32, 16, 4, 32, 8, 64, 16 };
// launch order of the transform sizes: longest-running shapes first (64-point, then 32-point ...)
static const uint8_t k_itx_launch_order[19] = { 4, 11, 12, 17, 18, 3, 9, 10, 15, 16, 2, 7, 8, 13, 14, 1, 5, 6, 0 };

struct Dav1dHipItxList {
    Dav1dHipItxTask *dev;
    size_t n;
    size_t off[20];   // bin b occupies [off[b], off[b+1])
};

struct Dav1dHipMcList {
    McTile *dev;      // tiles bin by bin (one launch per tile shape)
    size_t n;
    size_t off[16];   // 15 tile-shape bins: 3 * class(w in 4..64) + class(h in 4..16)
    McTile *dev_all;  // the same tiles, all shapes interleaved in source order (one launch for everything)
    McGroup *groups;
    size_t n_groups, n_fused;
    int max_ref;      // highest reference index any tile uses: checked against n_refs at run time
    McTile *host;     // host copy of `dev` in source order: regrouped per reference geometry at run time
    uint64_t geo_sig; // geometry the device copy is grouped for (0 = not yet)
};

struct Dav1dHipCompList {
    Dav1dHipCompTask *dev;
    size_t n;
    size_t n_first;   // tasks [0, n_first) run in the first launch, the BLEND_V tasks after them in a second one
};

struct Dav1dHipInterList {
    Dav1dHipMcList *mc;
    Dav1dHipCompList *comp;
    size_t n_fused;
    // with a picture geometry (recon lists): which launches write each 4x4 cell of a plane — bit b = the mc launch of tile
    // shape b, bit 15 = the compound / blend launch
    std::vector<uint16_t> writers[3];
    int cell_stride[3], stride_px[3];
};

struct Dav1dHipReconList {
    Dav1dHipInterList *inter;  // predictions that have no residual of their own shape (and everything when pairing is off)
    Dav1dHipItxList *itx;      // residuals without a prediction of their own shape
    uint16_t dep[19];          // per transform size: bits of the launches (see Dav1dHipInterList::writers) it has to wait for
    int stride_px[3];
    // paired blocks, per square size class 4x4 .. 64x64: tiles (1, 1, 1, 2, 4 per block) and transform tasks, device resident
    McTile *f_tiles[5];
    Dav1dHipItxTask *f_tasks[5];
    size_t f_n[5];
    int f_max_ref;
    bool wide_ok;              // every transform block starts at a multiple of min(its width, 8) pixels: the blocks may leave through
                               // tile_write_out (itx_body.h) in aligned row pieces.  Always so for AV1 geometry; checked because lists are an API
};

// Recon lists: a transform block that covers exactly one prediction block (same plane, position and size, square 4x4 ..
// 64x64) is paired with it; the pair runs in one wave (recon.hip) and the prediction never reaches the picture on its own.
struct ReconPairing {
    std::unordered_map<uint64_t, uint32_t> by_pos;      // plane << 32 | dst_off -> index of the (square) transform task there
    const Dav1dHipItxTask *itx;
    std::vector<char> taken;                            // per transform task: paired
    std::vector<McTile> tiles[5];                       // per size class: tiles of the paired blocks, block by block
    std::vector<uint32_t> itx_idx[5];                   // per size class: the transform task of each block
    int mask;                                           // size classes that pair (bit k: 4 << k pixels square)
    int stride_px[3];                                   // picture strides (pixels) of the geometry the list is made for
    std::vector<uint8_t> blend_cells[3];                // per plane: 4x4 cells a blend task writes
    int cell_stride[3];
    void block_blend(const Dav1dHipCompTask &k) {
        const int sp = stride_px[k.plane];
        if (sp <= 0) return;
        const int x = (int) (k.dst_off % (uint32_t) sp), y = (int) (k.dst_off / (uint32_t) sp);
        for (int cy = y >> 2; cy <= (y + k.h - 1) >> 2; cy++)
            for (int cx = x >> 2; cx <= (x + k.w - 1) >> 2; cx++) {
                const size_t i = (size_t) cy * cell_stride[k.plane] + cx;
                if (cx < cell_stride[k.plane] && i < blend_cells[k.plane].size()) blend_cells[k.plane][i] = 1;
            }
    }
    bool blended(int plane, uint32_t dst_off, int w, int h) const {
        const int sp = stride_px[plane];
        if (sp <= 0 || blend_cells[plane].empty()) return false;
        const int x = (int) (dst_off % (uint32_t) sp), y = (int) (dst_off / (uint32_t) sp);
        for (int cy = y >> 2; cy <= (y + h - 1) >> 2; cy++)
            for (int cx = x >> 2; cx <= (x + w - 1) >> 2; cx++) {
                const size_t i = (size_t) cy * cell_stride[plane] + cx;
                if (cx < cell_stride[plane] && i < blend_cells[plane].size() && blend_cells[plane][i]) return true;
            }
        return false;
    }
    // the transform task a prediction of this rectangle pairs with, or -1
    long find(int plane, uint32_t dst_off, int w, int h) {
        if (w != h || blended(plane, dst_off, w, h)) return -1;
        auto it = by_pos.find((uint64_t) plane << 32 | dst_off);
        if (it == by_pos.end() || taken[it->second]) return -1;
        const Dav1dHipItxTask &t = itx[it->second];
        return (t.tx <= 4 && (mask >> t.tx & 1) && (4 << t.tx) == w) ? (long) it->second : -1;
    }
};

bool itx_task_ok(const Dav1dHipItxTask &t);
void itx_fill_prefix(Dav1dHipItxTask &t);
int itx_path_key(const Dav1dHipItxTask &t);
int mc_task_valid(const Dav1dHipMcTask &t);
McRef mc_ref_of(const Dav1dHipMcTask &t);
void push_tiles(std::vector<McTile> *bins, const Dav1dHipMcTask &t, int kind, uint32_t dst_off, const Dav1dHipMcTask *second, int weight,
                std::vector<McTile> *single = nullptr);
int recon_fuse_mask(const Dav1dHipContext *c);
int tile_dim_class(int v);
// api_lists.hip, for the recon lists of api_recon.hip.  Hidden by name: the emulated build does not hide by default, and these were never exported.
#define LIST_LOCAL __attribute__((visibility("hidden")))
LIST_LOCAL int mc_fused_min_bin();          // DAV1D_HIP_MC_FUSED, read once
LIST_LOCAL int mc_regroup(Dav1dHipContext *c, Dav1dHipMcList *l, const DevPlanes *rp, int n_refs);
LIST_LOCAL int inter_list_create_geo(Dav1dHipContext *c, Dav1dHipInterList **out, const Dav1dHipMcTask *mc, size_t n_mc,
                                     const Dav1dHipCompTask *comp, size_t n_comp, const Dav1dHipPicture *geom, ReconPairing *pair = nullptr);
uint8_t *dav1d_hip_slab_get(Dav1dHipContext *c, size_t bytes, size_t *cap);      // chunk.hip: pinned host memory, recycled through the context
void dav1d_hip_slab_put(Dav1dHipContext *c, uint8_t *host, size_t cap);
