// Acquisition launch templates instantiated for the four-step FFT (sizes beyond one workgroup's LDS).
#include "acq_launch.h"

int gsdr_acq_impl::dispatch_four(gsdr_acq* a, const AcqView& v, const AcqOp& op)
{
    return a->variant >= 24 ? run_on(FourPkPlans{}, a, v, op) : run_on(FourPlans{}, a, v, op);
}
