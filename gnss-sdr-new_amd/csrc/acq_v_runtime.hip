// Acquisition launch templates instantiated for the runtime-planned LDS FFT (other 2^a 3^b 5^c sizes).
#include "acq_launch.h"

int gsdr_acq_impl::dispatch_runtime(gsdr_acq* a, const AcqView& v, const AcqOp& op)
{
    return run_on(RuntimePlans{}, a, v, op);
}
