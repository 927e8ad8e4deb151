// The Kalman-loop instances of trk_kernel (trk_kernel.h), in a translation unit of their
// own: with both loops in one unit the flagship DLL/PLL instance (gr_complex, float
// replicas) came out with one VGPR spilled, where it has none without them.
#include "trk_kernel.h"

namespace gsdr
{
trk::TrkKernel trk_kf_kernel(int item_type, bool pack)
{
    if (item_type == GSDR_ITEM_GR_COMPLEX) return pack ? trk_kernel<GSDR_ITEM_GR_COMPLEX, true, true> : trk_kernel<GSDR_ITEM_GR_COMPLEX, false, true>;
    if (item_type == GSDR_ITEM_CSHORT) return pack ? trk_kernel<GSDR_ITEM_CSHORT, true, true> : trk_kernel<GSDR_ITEM_CSHORT, false, true>;
    return pack ? trk_kernel<GSDR_ITEM_IBYTE, true, true> : trk_kernel<GSDR_ITEM_IBYTE, false, true>;
}
}  // namespace gsdr
