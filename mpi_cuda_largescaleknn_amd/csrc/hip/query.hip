// Foreign queries (points that are not the index's own): where a group of 64 curve-sorted
// queries lies in the index. The k-NN kernels' foreign forms (knn_rows NT = 4, knn_grid
// FOREIGN) take the walk's own bucket and the points their first range is estimated from
// out of the data there, never from the neighbouring queries.
#include "dev.h"

namespace {

// One thread per query group: the last bucket whose first key is <= the group's median key
// (bkeys is non-decreasing: the index's points are sorted by key, and the refinement of
// over-full cells only reorders points of equal keys). A key below every bucket's: bucket 0.
__global__ __launch_bounds__(256) void locate_groups_kernel(const uint32_t *__restrict__ qkeys, int64_t nq,
                                                            const uint32_t *__restrict__ bkeys, int64_t nb,
                                                            uint32_t *__restrict__ out, int64_t ngroups) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= ngroups) return;
  const int64_t q0 = g * lsk::kBucket;
  const int64_t nvalid = nq - q0 < lsk::kBucket ? nq - q0 : lsk::kBucket;
  const uint32_t key = qkeys[q0 + nvalid / 2];  // (nvalid >= 1: q0 + nvalid / 2 < nq)
  int64_t lo = 0, hi = nb;                      // first b in [0, nb] with bkeys[b] > key
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (bkeys[mid] <= key)
      lo = mid + 1;
    else
      hi = mid;
  }
  out[g] = (uint32_t)(lo > 0 ? lo - 1 : 0);
}

}  // namespace

extern "C" int lsk_hip_locate_groups(const uint32_t *qkeys, int64_t nq, const uint32_t *bkeys, int64_t nb,
                                     uint32_t *out, void *stream) {
  if (nq < 0 || nb < 0 || nb >= ((int64_t)1 << 32)) {
    lsk::set_last_error("locate_groups: nq >= 0 and 0 <= nb < 2^32");
    return 1;
  }
  const int64_t ngroups = (nq + lsk::kBucket - 1) / lsk::kBucket;
  if (ngroups == 0) return 0;
  if (nb == 0) return (int)lsk_fill32(out, 0u, ngroups, (hipStream_t)stream);
  locate_groups_kernel<<<lsk_blocks(ngroups, 256), 256, 0, (hipStream_t)stream>>>(qkeys, nq, bkeys, nb, out,
                                                                                  ngroups);
  LSK_CHECK_LAUNCH("locate_groups");
  return 0;
}
