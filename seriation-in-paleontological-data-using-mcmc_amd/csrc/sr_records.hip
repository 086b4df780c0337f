/*
 * sr_records.hip -- the record view (sr_records.h): the records and the per-chain offsets brought to the GPU once,
 * for every analysis that reads them.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "sr_records.h"
#include "sr_analysis.h"

extern "C" int sr_recview_device(sr_recview *v, int device, void *stream, const int16_t *d_rec, const long long *off,
                                 int n_sel, int count, long long row_stride)
{
  int rc = 0;
  long long *d_off = nullptr;
  if (!v) return -1;
  memset(v, 0, sizeof(*v));
  if (!d_rec || !off || n_sel <= 0 || count < 0) return -1;
  HIPCHK(hipSetDevice(device));
  HIPCHK(hipMalloc(&d_off, sizeof(long long) * n_sel));
  HIPCHK(hipMemcpy(d_off, off, sizeof(long long) * n_sel, hipMemcpyHostToDevice));
  v->device = device; v->stream = stream; v->rec = d_rec; v->chain_off = d_off;
  v->n_sel = n_sel; v->count = count; v->row_stride = row_stride;
  d_off = nullptr;
done:
  if (d_off) (void)hipFree(d_off);
  return rc;
}

extern "C" int sr_recview_host(sr_recview *v, int device, const int16_t *ab_pi, int n_sel, int count, long long W)
{
  int rc = 0;
  int16_t *d_rec = nullptr;
  long long *off = nullptr;
  if (!v) return -1;
  memset(v, 0, sizeof(*v));
  if (!ab_pi || n_sel <= 0 || count < 0 || W < 1) return -1;
  const size_t bytes = (size_t)n_sel * count * W * sizeof(int16_t);
  off = (long long *)malloc(sizeof(long long) * n_sel);
  if (!off) return -4;
  for (int k = 0; k < n_sel; ++k) off[k] = (long long)k * count * W;
  HIPCHK(hipSetDevice(device));
  /* 16 bytes more than the rows: no kernel reads past the last row (sr_post_kernel, the one that takes a view of
     no rows, clamps every sample index to the last sample and loads nothing when there is none); the pad only keeps
     the allocation, and so rec, from being empty when count == 0 */
  HIPCHK(hipMalloc(&d_rec, bytes + 16));
  if (bytes) HIPCHK(hipMemcpy(d_rec, ab_pi, bytes, hipMemcpyHostToDevice));
  rc = sr_recview_device(v, device, nullptr, d_rec, off, n_sel, count, W);
  if (!rc) {
    v->owns_rec = 1;
    d_rec = nullptr;
  }
done:
  if (d_rec) (void)hipFree(d_rec);
  free(off);
  return rc;
}

extern "C" void sr_recview_release(sr_recview *v)
{
  if (!v) return;
  if (v->chain_off) (void)hipFree((void *)v->chain_off);
  if (v->owns_rec && v->rec) (void)hipFree((void *)v->rec);
  memset(v, 0, sizeof(*v));
}
