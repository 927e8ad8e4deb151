// Kf_Conf mirror (src/algorithms/tracking/libs/kf_conf.h, kf_conf.cc): the Tracking_XX.* keys that
// drive kf_tracking.  The keys it shares with Dll_Pll_Conf are read by that class (the Kalman loop
// ignores the loop bandwidths, filter orders, enable_fll_* and carrier_aiding among them); on top come
// the ten Kalman values and the reference's own defaults: the dump file name and
// bit_synchronization_time_limit_s = pull_in_time_s + 60 (kf_conf.cc:91-92).  The object is a
// Dll_Pll_Conf with `kf` set, which is what the tracking blocks look at (gsdr_trk_set_kf).
#ifndef GSDR_HOST_KF_CONF_H
#define GSDR_HOST_KF_CONF_H

#include <string>

#include "dll_pll_conf.h"

class Kf_Conf : public Dll_Pll_Conf
{
public:
    Kf_Conf();
    void SetFromConfiguration(const ConfigurationInterface* configuration, const std::string& role);
};

#endif
