// Acquisition launch templates instantiated for the compile-time FFT plans (1 ms at 2/4/8/16 Msps).
#include "acq_launch.h"

int gsdr_acq_impl::dispatch_static(gsdr_acq* a, const AcqView& v, const AcqOp& op)
{
    return run_on(StaticPlans{}, a, v, op);
}
