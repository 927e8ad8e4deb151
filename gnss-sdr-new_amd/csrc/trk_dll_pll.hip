// The DLL/PLL-loop instances of trk_kernel (trk_kernel.h).
#include "trk_kernel.h"

namespace gsdr
{
trk::TrkKernel trk_dll_pll_kernel(int item_type, bool pack)
{
    if (item_type == GSDR_ITEM_GR_COMPLEX) return pack ? trk_kernel<GSDR_ITEM_GR_COMPLEX, true, false> : trk_kernel<GSDR_ITEM_GR_COMPLEX, false, false>;
    if (item_type == GSDR_ITEM_CSHORT) return pack ? trk_kernel<GSDR_ITEM_CSHORT, true, false> : trk_kernel<GSDR_ITEM_CSHORT, false, false>;
    return pack ? trk_kernel<GSDR_ITEM_IBYTE, true, false> : trk_kernel<GSDR_ITEM_IBYTE, false, false>;
}
}  // namespace gsdr
