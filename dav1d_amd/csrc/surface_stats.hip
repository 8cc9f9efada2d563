// Per-picture light statistics on the device and the tone part of a live handle replaced in place (dav1d_hip_picture_light_stats and the
// dav1d_hip_light_stats_* calls, dav1d_hip_colour_update_tone; include/dav1d_hip.h).  The histogram is indexed like the gain of a
// toned handle (step 1b of 10.12): h, the binary16 pattern of the clamped luminance of a pixel of the crop window W at W's own size.  Every count
// is an integer, so kernel, emulated build and numpy agree to the last one whatever the order of the adds.
//
// The pixels are the source-resolution loader's (surface_source.h, the one of surface_linear.hip): a wave takes a 64 x 8 cell of W's luma plane from a
// multiple of 8 on both axes, 8 rows x 8 units of 8 samples; a lane loads its luma unit and the chroma under it, runs rgbx_unit of surface_common.h
// on them and has the integers of 8 pixels.  Nothing is stored.  Per pixel: lin three times, step 1b's Y, x and h, and one count.
// LDS is the histogram — 15,361 bins of 32 bits and four words of side counters — and lin behind it, 16 KiB at 12 bits: 77,856 bytes, static, more
// than the 64 KiB a launch gets on older parts and what a gfx950 launch may declare; two workgroups a CU either way (155,712 of 163,840 bytes), which is
// why a workgroup is eight waves (four a SIMD).  lin was read from the handle in global memory first, as gain is: three gathers a pixel at addresses
// the picture chooses, 100 M of them at 8K, bound the kernel at 1.5 times the full-size colour export.  A workgroup's share of a
// picture stays below 2^32 pixels (the host sees to it), so a bin cannot wrap.
// Contention.  Same-address LDS atomics of a wave serialise, and flat areas put every lane into one bin.  Per pixel slot the wave compares with the
// bin of its first lane that still has a pixel and adds the population count of the lanes that agree, once; a
// second round does the same for what is left (a picture of two levels is through after two adds); the lanes left after that add one each — in
// noise they hit different addresses.
// Flush.  The grid is bounded (ST_GROUPS workgroups that loop over cells), so the flushes do not grow with the picture: the nonzero bins go to the
// accumulator with 64-bit atomic adds, the three counters with one each per workgroup, max_light as an order-preserving unsigned with one atomic
// maximum per workgroup.
#include "surface_reduce.h"
#include "surface_colour.h"
#include "surface_source.h"
#include <math.h>
#include <stddef.h>

struct Dav1dHipLightStats {
    unsigned long long *dev;          // the words of Dav1dHipLightStatsData; the place of max_light holds its key (0: nothing counted)
    int device;
};

namespace {

constexpr int ST_WAVES = 8, ST_THREADS = 64 * ST_WAVES;
constexpr int ST_BINS = DAV1D_HIP_COLOUR_ENC_N;
constexpr unsigned ST_GROUPS = 2 * MI355X_CUS;          // as many as are resident at once
constexpr int ST_HIST_AT = 4;                          // words of the accumulator in front of hist: n, n_above, n_nonpos, the key of max_light

static_assert(offsetof(Dav1dHipLightStatsData, max_light) == 24 && offsetof(Dav1dHipLightStatsData, hist) == 8 * ST_HIST_AT, "the accumulator is the record");
static_assert(sizeof(Dav1dHipLightStatsData) == 8 * (ST_HIST_AT + ST_BINS), "the accumulator is the record");

struct alignas(16) StatsLds {
    uint32_t hist[ST_BINS];
    uint32_t n, above, nonpos, maxkey;
    alignas(16) float lin[1 << 12];          // the handle's, the first 1 << bpc entries
};
static_assert(2 * sizeof(StatsLds) <= LDS_PER_CU, "two workgroups a CU");

struct StatsArgs {
    const void *s;                  // the luma plane
    int sstride, swide, pw;         // pixels per row; one vector load per unit; visible samples per row
    const void *cs[2];              // U, V
    int cstride, cswide, cpw;
    int cx0, cy0, ccw, cch;         // W's chroma planes: cl() clamps against these
    RgbArgs c;                      // the colour part
    int pos, hf, vf;
    int x0, x1, y0, y1;             // the columns and rows of the picture that are counted
    int ux0, ry0;                   // the first cell's corner: multiples of 8 at or in front of them
    int n_cx;
    unsigned n_cells;
    const float *lin;
    int mask;                       // entries of lin - 1
    float k[3];
    unsigned long long *acc;
};

// a float as an unsigned that orders like it (-0.0 below +0); 0 is the key of no finite value
__device__ __forceinline__ unsigned key_of(const float f)
{
    unsigned b;
    __builtin_memcpy(&b, &f, 4);
    return b & 0x80000000u ? ~b : b | 0x80000000u;
}
inline float value_of_key(const unsigned key)
{
    if (!key) return -INFINITY;
    const unsigned b = key & 0x80000000u ? key ^ 0x80000000u : ~key;
    float f;
    memcpy(&f, &b, 4);
    return f;
}

// the two atomics the emulated build's runtime does not have (its lanes run one after the other: a plain read and write is atomic there)
__device__ __forceinline__ void add_u64(unsigned long long *const p, const unsigned long long v)
{
#ifdef DAV1D_HIP_EMU
    *p += v;
#else
    atomicAdd(p, v);
#endif
}
__device__ __forceinline__ void max_u32(unsigned *const p, const unsigned v)
{
#ifdef DAV1D_HIP_EMU
    if (v > *p) *p = v;
#else
    atomicMax(p, v);
#endif
}

// one pixel slot of a wave into the histogram: every lane of the wave calls, `valid` says whether it has a pixel
__device__ __forceinline__ void count_bin(StatsLds &L, const unsigned h, const bool valid, const int lane)
{
    unsigned long long todo = __ballot(valid);
#pragma unroll
    for (int round = 0; round < 2; round++) {
        if (!todo) break;          // (uniform in the wave)
        const int leader = __ffsll(todo) - 1;
        const unsigned hl = (unsigned) __shfl((int) h, leader);
        const unsigned long long same = __ballot(((todo >> lane) & 1) && h == hl);
        if (lane == leader) atomicAdd(&L.hist[hl], (unsigned) __popcll(same));
        todo &= ~same;
    }
    if ((todo >> lane) & 1) atomicAdd(&L.hist[h], 1u);
}

template <typename pixel, bool TILED, int SSH, int SSV>
__global__ __launch_bounds__(ST_THREADS) void surface_stats_kernel(const StatsArgs a0)
{
    __shared__ StatsLds L;
    typedef Piece<8 * sizeof(pixel)> piece_t;
    const int tid = (int) threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane >> 3, c = lane & 7;
    for (int i = tid; i < ST_BINS; i += ST_THREADS) L.hist[i] = 0;
    if (tid == 0) L.n = L.above = L.nonpos = L.maxkey = 0;
    StatsArgs a = a0;
    a.s = in_device_memory(a.s); a.cs[0] = in_device_memory(a.cs[0]); a.cs[1] = in_device_memory(a.cs[1]);
    {
        const uint4 *const src = reinterpret_cast<const uint4 *>(in_device_memory(a.lin));
        uint4 *const dst = reinterpret_cast<uint4 *>(L.lin);
        for (int i = tid; i < (a.mask + 1) / 4; i += ST_THREADS) dst[i] = src[i];
    }
    __syncthreads();          // (before any lane reads a table or adds to a bin)
    const float *const lin = L.lin;
    unsigned n = 0, above = 0, nonpos = 0, maxkey = 0;
    const unsigned step = (unsigned) gridDim.x * ST_WAVES;
    // (the loop is uniform in the wave: no lane leaves before the last exchange of count_bin)
    for (unsigned cell = (unsigned) blockIdx.x * ST_WAVES + (unsigned) wave; cell < a.n_cells; cell += step) {
        const int cy = (int) (cell / (unsigned) a.n_cx), cx = (int) (cell - (unsigned) cy * (unsigned) a.n_cx);
        const int x = a.ux0 + cx * 64 + c * 8, y = a.ry0 + cy * 8 + r;
        const bool ok = x < a.x1 && y >= a.y0 && y < a.y1;
        int R[8], G[8], B[8];
        if (ok) {
            const piece_t v = load8<pixel, TILED>(a.s, a.sstride, x, y, a.pw - x, a.swide);
            LinChroma<pixel> k;
            if (!a.c.mono) lin_chroma_load<pixel, TILED, SSH, SSV>(a, x, y, k);
            uint32_t P[8];
            lin_chroma_taps<pixel, SSH>(a, x, k, P);
            uint16_t sy[8];
#pragma unroll
            for (int e = 0; e < 8; e++) sy[e] = (uint16_t) sample_of<pixel>(v, e);
            rgbx_unit<SSH, RgbRaw>(a.c, RgbRaw(), sy, P, a.hf != 0, R, G, B);
        }
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const bool valid = ok && x + e >= a.x0 && x + e < a.x1;
            unsigned h = 0;
            if (valid) {
                const float l0 = lin[R[e] & a.mask], l1 = lin[G[e] & a.mask], l2 = lin[B[e] & a.mask];
                const float Y = row_5r(a.k, l0, l1, l2);
                const float xc = Y > 0.0f ? (Y < 1.0f ? Y : 1.0f) : 0.0f;          // (a NaN fails the first comparison)
                h = dv::f32_to_f16_bits(xc) & 0x7fffu;
                h = h < 0x3c00u ? h : 0x3c00u;          // (xc is in [+0, 1]: neither changes anything, and the add stays inside the histogram whatever a compiler makes of the clamp)
                n++;
                above += Y > 1.0f;
                nonpos += !(Y > 0.0f);
                const unsigned k0 = key_of(l0), k1 = key_of(l1), k2 = key_of(l2);
                const unsigned km = k0 > k1 ? (k0 > k2 ? k0 : k2) : (k1 > k2 ? k1 : k2);
                maxkey = maxkey > km ? maxkey : km;
            }
            count_bin(L, h, valid, lane);
        }
    }
    // ---- the wave's counters, the workgroup's, the accumulator's
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        n += (unsigned) __shfl_xor((int) n, m);
        above += (unsigned) __shfl_xor((int) above, m);
        nonpos += (unsigned) __shfl_xor((int) nonpos, m);
        const unsigned o = (unsigned) __shfl_xor((int) maxkey, m);
        maxkey = maxkey > o ? maxkey : o;
    }
    if (lane == 0 && n) {
        atomicAdd(&L.n, n); atomicAdd(&L.above, above); atomicAdd(&L.nonpos, nonpos);
        max_u32(&L.maxkey, maxkey);
    }
    __syncthreads();
    unsigned long long *const acc = in_device_memory(a.acc);
    for (int i = tid; i < ST_BINS; i += ST_THREADS) {
        const uint32_t v = L.hist[i];
        if (v) add_u64(&acc[ST_HIST_AT + i], (unsigned long long) v);
    }
    if (tid == 0 && L.n) {
        add_u64(&acc[0], (unsigned long long) L.n);
        if (L.above) add_u64(&acc[1], (unsigned long long) L.above);
        if (L.nonpos) add_u64(&acc[2], (unsigned long long) L.nonpos);
        max_u32(reinterpret_cast<unsigned *>(&acc[3]), L.maxkey);          // (the low word: where max_light lies)
    }
}

bool finite_f32(const float f) { uint32_t x; memcpy(&x, &f, 4); return (x & 0x7f800000u) != 0x7f800000u; }

// the kernel's arguments for luma rows [row0, row1) of the crop of a checked call
template <typename pixel, bool TILED>
StatsArgs make_stats_args(const Dav1dHipPicture *const src, void *const *const planes, const ScaleGeom &g, const Dav1dHipSurface &as, const int chroma_pos,
                          const int row0, const int row1, const Dav1dHipColour *const h, const float *const k, unsigned long long *const acc, unsigned long long *const n_cells)
{
    const int load_align = 8 * (int) sizeof(pixel);
    StatsArgs a = StatsArgs();
    a.s = planes[0];
    a.sstride = (int) (src->p[0].stride / (ptrdiff_t) sizeof(pixel));
    a.swide = TILED || aligned_to(planes[0], src->p[0].stride, load_align);
    a.pw = src->p[0].w;
    if (!g.mono) {
        a.cs[0] = planes[1]; a.cs[1] = planes[2];
        a.cstride = (int) (src->p[1].stride / (ptrdiff_t) sizeof(pixel));
        a.cswide = TILED || (aligned_to(planes[1], src->p[1].stride, load_align) && aligned_to(planes[2], src->p[2].stride, load_align));
        a.cpw = src->p[1].w;
    }
    a.cx0 = g.x0 >> g.ss_hor; a.cy0 = g.y0 >> g.ss_ver;
    a.ccw = (g.w + g.ss_hor) >> g.ss_hor; a.cch = (g.h + g.ss_ver) >> g.ss_ver;
    rgb_set_matrix(a.c, &as, src->bpc, g.mono);
    a.pos = chroma_pos; a.hf = g.ss_hor && chroma_pos; a.vf = g.ss_ver && chroma_pos;
    a.x0 = g.x0; a.x1 = g.x0 + g.w; a.y0 = g.y0 + row0; a.y1 = g.y0 + row1;
    a.ux0 = a.x0 & ~7; a.ry0 = a.y0 & ~7;
    a.n_cx = (a.x1 - a.ux0 + 63) / 64;
    *n_cells = (unsigned long long) a.n_cx * (unsigned long long) ((a.y1 - a.ry0 + 7) / 8);
    a.n_cells = (unsigned) *n_cells;
    a.lin = reinterpret_cast<const float *>(h->dev); a.mask = (1 << h->bpc) - 1;
    memcpy(a.k, k, sizeof(a.k));
    a.acc = acc;
    return a;
}

template <typename pixel, bool TILED>
int launch_stats(Dav1dHipContext *const c, const Dav1dHipPicture *const src, void *const *const planes, const ScaleGeom &g, const Dav1dHipSurface &as,
                 const int chroma_pos, const int row0, const int row1, const Dav1dHipColour *const h, const float *const k, unsigned long long *const acc)
{
    unsigned long long n_cells;
    const StatsArgs a = make_stats_args<pixel, TILED>(src, planes, g, as, chroma_pos, row0, row1, h, k, acc, &n_cells);
    if (n_cells >> 32) return -EINVAL;          // (2^41 pixels: no picture)
    // a cell a wave while there are fewer cells than resident waves, then ST_GROUPS workgroups that loop — more only where a workgroup's share
    // would reach 2^32 pixels, which a bin of 32 bits could not count
    unsigned long long groups = (n_cells + ST_WAVES - 1) / ST_WAVES;
    if (groups > ST_GROUPS) groups = ST_GROUPS;
    while ((n_cells + groups * ST_WAVES - 1) / (groups * ST_WAVES) * (ST_WAVES * 512ull) >> 32) groups *= 2;
    const dim3 grid((unsigned) groups), wg(ST_THREADS);
    if (g.ss_ver) hipLaunchKernelGGL((surface_stats_kernel<pixel, TILED, 1, 1>), grid, wg, 0, c->stream, a);
    else if (g.ss_hor) hipLaunchKernelGGL((surface_stats_kernel<pixel, TILED, 1, 0>), grid, wg, 0, c->stream, a);
    else hipLaunchKernelGGL((surface_stats_kernel<pixel, TILED, 0, 0>), grid, wg, 0, c->stream, a);
    return hip_rc(hipGetLastError());
}

} // namespace

extern "C" int dav1d_hip_light_stats_create(Dav1dHipContext *c, Dav1dHipLightStats **out)
{
    if (!c || !out) return -EINVAL;
    *out = nullptr;
    Dav1dHipLightStats *const s = new (std::nothrow) Dav1dHipLightStats();
    if (!s) return -ENOMEM;
    s->device = c->device;
    int cur = -1, rc = 0;
    (void) hipGetDevice(&cur);
    if (cur != c->device && hipSetDevice(c->device) != hipSuccess) rc = -ENODEV;
    if (!rc) rc = hip_rc(hipMalloc((void **) &s->dev, sizeof(Dav1dHipLightStatsData)));
    if (!rc) {
        rc = hip_rc(hipMemsetAsync(s->dev, 0, sizeof(Dav1dHipLightStatsData), c->stream));
        if (rc) (void) hipFree(s->dev);
    }
    if (cur >= 0 && cur != c->device) (void) hipSetDevice(cur);
    if (rc) { delete s; return rc; }
    __atomic_fetch_add(&dav1d_hip_live[4], 1, __ATOMIC_RELAXED);
    *out = s;
    return 0;
}

extern "C" int dav1d_hip_light_stats_destroy(Dav1dHipContext *c, Dav1dHipLightStats *s)
{
    if (!s) return 0;
    if (c) (void) hipStreamSynchronize(c->stream);
    const int rc = hip_rc(hipFree(s->dev));
    delete s;
    __atomic_fetch_sub(&dav1d_hip_live[4], 1, __ATOMIC_RELAXED);
    return rc;
}

extern "C" long long dav1d_hip_light_stats_alive(void) { return __atomic_load_n(&dav1d_hip_live[4], __ATOMIC_RELAXED); }

extern "C" int dav1d_hip_light_stats_reset(Dav1dHipContext *c, Dav1dHipLightStats *s)
{
    if (!c || !s) return -EINVAL;
    if (s->device != c->device) return -EXDEV;
    return hip_rc(hipMemsetAsync(s->dev, 0, sizeof(Dav1dHipLightStatsData), c->stream));
}

extern "C" int dav1d_hip_light_stats_read(Dav1dHipContext *c, const Dav1dHipLightStats *s, Dav1dHipLightStatsData *out)
{
    if (!c || !s || !out) return -EINVAL;
    if (s->device != c->device) return -EXDEV;
    const int rc = hip_rc(hipMemcpyAsync(out, s->dev, sizeof(*out), hipMemcpyDeviceToHost, c->stream));
    const int rs = hip_rc(hipStreamSynchronize(c->stream));
    if (rc || rs) return rc ? rc : rs;
    unsigned key;
    memcpy(&key, &out->max_light, 4);
    out->max_light = value_of_key(key);
    return 0;
}

extern "C" int dav1d_hip_picture_light_stats(Dav1dHipContext *c, Dav1dHipLightStats *s, const Dav1dHipPicture *src, const Dav1dHipSurfaceRect *crop,
                                             int matrix, int full_range, int chroma_pos, const Dav1dHipColour *colour, const float k[3], int row0, int row1)
{
    if (!c || !s || !src || !colour || !k) return -EINVAL;
    // what the linear-light export refuses about the picture, the crop, the matrix and chroma_pos: asked of it, for a float surface of the crop's size
    Dav1dHipSurface as = Dav1dHipSurface();
    as.format = DAV1D_HIP_SURFACE_RGB_PLANAR; as.sample = DAV1D_HIP_SAMPLE_F32;
    as.w = crop ? (crop->w > 0 ? crop->w : 1) : src->p[0].w; as.h = crop ? (crop->h > 0 ? crop->h : 1) : src->p[0].h;          // (a crop without a size is the geometry check's to refuse)
    for (int pl = 0; pl < 3; pl++) { as.data[pl] = &as; as.stride[pl] = (ptrdiff_t) 4 * (as.w > 0 ? as.w : 1); }               // (never written, never read)
    as.matrix = matrix; as.full_range = full_range;
    Dav1dHipRgbParams p = Dav1dHipRgbParams();
    p.chroma_pos = chroma_pos;
    SurfaceCall call;
    ScaleGeom g;
    if (const int rc = reduced_args_check(&as, src, crop, p, DAV1D_HIP_RESIZE_BILINEAR, row0, row1, &call, &g)) return rc;
    for (int i = 0; i < 3; i++) if (!finite_f32(k[i])) return -EINVAL;
    if (colour->bpc != src->bpc) return -EINVAL;
    if (const int rc = pictures_on_device(c, src, 1)) return rc;
    if (colour->device != c->device || s->device != c->device) return -EXDEV;
    if (call.row1 <= call.row0) return 0;
    const CallTimer t(c);
    return t.done(with_pixel_state(src->bpc, call.tiled, [&](auto px, auto state) {
        return launch_stats<decltype(px), decltype(state)::value>(c, src, call.planes, g, as, chroma_pos, call.row0, call.row1, colour, k, s->dev);
    }));
}

// ---- the host helpers: integers, but for the one sum in double

extern "C" int dav1d_hip_light_stats_rank(const Dav1dHipLightStatsData *d, uint64_t rank, int *h)
{
    if (!d || !h || rank == 0 || rank > d->n) return -EINVAL;
    uint64_t sum = 0;
    for (int i = 0; i < ST_BINS; i++) {
        sum += d->hist[i];
        if (sum >= rank) { *h = i; return 0; }
    }
    return -EINVAL;          // (a record whose bins do not add up to n)
}

extern "C" double dav1d_hip_light_stats_mean(const Dav1dHipLightStatsData *d)
{
    if (!d || !d->n) return 0.0;
    double sum = 0.0;
    for (int i = 0; i < ST_BINS; i++)          // ascending: the order is part of the definition
        sum += (double) d->hist[i] * (i < 0x400 ? ldexp((double) i, -24) : ldexp((double) (0x400 | (i & 0x3ff)), (i >> 10) - 25));
    return sum / (double) d->n;
}

// ---- the tone part of a live handle, replaced in stream order

extern "C" int dav1d_hip_colour_update_tone(Dav1dHipContext *c, Dav1dHipColour *h, const Dav1dHipColourTone *t)
{
    if (!c || !h || !t) return -EINVAL;
    if (!h->has_tone) return -EINVAL;
    if (!t->gain) return -EINVAL;
    for (int i = 0; i < 3; i++) if (!finite_f32(t->k[i])) return -EINVAL;
    for (int i = 0; i < DAV1D_HIP_COLOUR_ENC_N; i++) if ((t->gain[i] & 0x7c00) == 0x7c00) return -EINVAL;
    if (h->device != c->device) return -EXDEV;
    // the caller's array may go away on return: the copy leaves from a slot of the staging ring, which is free again once the copy has run
    Dav1dHipContext::BatchStage *s;
    if (const int rc = batch_stage_take(c, ENC_BYTES, &s)) return rc;
    memcpy(s->host, t->gain, DAV1D_HIP_COLOUR_ENC_N * sizeof(uint16_t));
    memset(s->host + DAV1D_HIP_COLOUR_ENC_N * sizeof(uint16_t), 0, ENC_BYTES - DAV1D_HIP_COLOUR_ENC_N * sizeof(uint16_t));
    const int rc = hip_rc(hipMemcpyAsync(h->dev + h->gain_off, s->host, ENC_BYTES, hipMemcpyHostToDevice, c->stream));
    (void) hipEventRecord(s->done, c->stream);
    s->busy = true;
    if (!rc) memcpy(h->ky, t->k, sizeof(h->ky));          // (a launch takes ky with it: the ones enqueued from here on take the new)
    return rc;
}
