// Many scaled tensor-ready exports in one launch: dav1d_hip_surface_export_rgb_scaled_batch (include/dav1d_hip.h).  Item i of a batch
// gets the bytes dav1d_hip_surface_export_rgb_scaled(c, &dst[i], src[i], crop ? &crop[i] : NULL, params, 0, dst[i].h) writes: the pixel work is that
// call's, scale_rgbx_cell of surface_common.h, and nothing here restates it.
//
//   table   one record per item: the ScaleRgbxArgs the single call would hand its kernel, and the output functor of the item's bit depth (10 and 12
//           bit sources may share a batch; 1 / max, the MSB16 shift and alpha differ between them).  Behind the records a prefix of workgroup counts:
//           first[k] = workgroups of the items before k, first[n] = all of them.
//   search  the grid is first[n] workgroups, no more: a whole picture next to thumbnails launches no empty ones.  A workgroup finds its item as the
//           last k with first[k] <= blockIdx.x, by bisection (10 steps at 1024 items), and runs cell blockIdx.x - first[k] of it.  blockIdx.x, the
//           table and the prefix (const __restrict__ kernel arguments) are uniform: the search and the record are scalar loads, the record stays
//           in SGPRs as the single call's by-value argument does.
//   states  the picture state (raster planes / tiled twin) is a template parameter of the loads, so a batch that mixes them is two launches, each
//           over its own slice of the table, between one pair of timing events.
//   staging the table is written into pinned host memory and copied to device memory on the context's stream.  Both belong to one of a ring of
//           slots of the context, each guarded by an event recorded behind the launches that read it: the call returns at once, the caller's arrays
//           are free, and a slot is waited for only when all of them are still in flight.  Slots grow on demand and are freed by dav1d_hip_close
//           (an outgrown one as well: hipFree waits for the device, capi.h TaskBuf).
// The host side of all of it — the front of the entry point, the table, the slot, the launches and the events — is surface_batch.h's, which the
// resized, reduced and colour-managed batches run through as well.
#include "surface_batch.h"

extern "C" int dav1d_hip_surface_export_rgb_scaled_batch(Dav1dHipContext *c, int n, const Dav1dHipSurface *dst, const Dav1dHipPicture *const *src,
                                                         const Dav1dHipSurfaceRect *crop, const Dav1dHipRgbParams *params, int *bad_item)
{
    return export_batch_call<false>(c, n, dst, src, crop, params, 0, bad_item);
}
