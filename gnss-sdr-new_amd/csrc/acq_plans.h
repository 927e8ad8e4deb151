// The FFT plans of the acquisition engine, gsdr_acq::variant -> plan type, listed
// once: choose_variant (acq.hip) takes sizes, workgroup widths and radices from
// these types, the acq_v_*.hip units instantiate the launch templates for them.
//   1-4    compile-time LDS plans for the sample rates GNSS front-ends use
//          (2/4/8/16 Msps at 1 ms, acq_v_static.hip)
//   10-12  runtime LDS plans for every other 2^a 3^b 5^c size (acq_v_runtime.hip)
//   20/22  the runtime four-step beyond one workgroup's LDS, N = R * N2 with a runtime
//          LDS sub-plan (acq_v_four.hip; GSDR_ACQ_FOUR_GENERIC=1 forces it)
//   24-27  the packed four-step (FourStepPkPlan) for the sizes of the GNSS
//          configurations beyond one workgroup's LDS: Galileo E1 4 / 8 ms at 8 Msps,
//          4 ms at 25 Msps, 1 ms at 25 Msps (acq_v_four.hip)
#pragma once
#include "fft_4step.h"
#include "fft_lds.h"
#include "fft_pk.h"

namespace gsdr_acq_impl
{

template <int ID, class PT>
struct PlanId
{
    static constexpr int id = ID;
    using type = PT;
};

template <class... E>
struct PlanList
{
};

// f(PlanId) for the entries in order until one returns true; false when none does.
template <class... E, class F>
bool find_plan(PlanList<E...>, F&& f)
{
    return (f(E{}) || ...);
}

using gsdr::fft::FourStepPkPlan;
using gsdr::fft::FourStepPlan;
using gsdr::fft::RuntimePlan;
using gsdr::fft::StaticPlan;
using gsdr::pk::PkPlan;

using StaticPlans = PlanList<PlanId<1, StaticPlan<256, 20, 20, 10>>, PlanId<2, StaticPlan<512, 20, 20, 20>>,
    PlanId<3, StaticPlan<1024, 16, 10, 10, 10>>, PlanId<4, StaticPlan<256, 20, 10, 10>>>;
using RuntimePlans = PlanList<PlanId<10, RuntimePlan<256>>, PlanId<11, RuntimePlan<512>>, PlanId<12, RuntimePlan<1024>>>;
using FourPlans = PlanList<PlanId<20, FourStepPlan<256>>, PlanId<22, FourStepPlan<1024>>>;
using FourPkPlans = PlanList<PlanId<24, FourStepPkPlan<8, PkPlan<256, 1, 25, 16, 10>>>,
    PlanId<25, FourStepPkPlan<16, PkPlan<256, 1, 25, 16, 10>>>, PlanId<26, FourStepPkPlan<25, PkPlan<256, 1, 25, 16, 10>>>,
    PlanId<27, FourStepPkPlan<5, PkPlan<256, 1, 25, 20, 10>>>>;

}  // namespace gsdr_acq_impl
