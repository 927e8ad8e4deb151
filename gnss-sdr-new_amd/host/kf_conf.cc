#include "kf_conf.h"

Kf_Conf::Kf_Conf()
{
    kf = true;
    gsdr_trk_kf_conf_default(&kf_conf);
    dump_filename = "./Kf_dump.dat";
    bit_synchronization_time_limit_s = 70U;
}

void Kf_Conf::SetFromConfiguration(const ConfigurationInterface* configuration, const std::string& role)
{
    const std::string dump_default = dump_filename;
    Dll_Pll_Conf::SetFromConfiguration(configuration, role);
    dump_filename = configuration->property(role + ".dump_filename", dump_default);
    bit_synchronization_time_limit_s = pull_in_time_s + 60U;  // kf_conf.cc:92: no key of its own
    // measurement covariances (R), system covariances (Q), initial covariances (P0): kf_conf.cc:120-133
    kf_conf.code_disc_sd_chips = configuration->property(role + ".code_disc_sd_chips", kf_conf.code_disc_sd_chips);
    kf_conf.carrier_disc_sd_rads = configuration->property(role + ".carrier_disc_sd_rads", kf_conf.carrier_disc_sd_rads);
    kf_conf.code_phase_sd_chips = configuration->property(role + ".code_phase_sd_chips", kf_conf.code_phase_sd_chips);
    kf_conf.carrier_phase_sd_rad = configuration->property(role + ".carrier_phase_sd_rad", kf_conf.carrier_phase_sd_rad);
    kf_conf.carrier_freq_sd_hz = configuration->property(role + ".carrier_freq_sd_hz", kf_conf.carrier_freq_sd_hz);
    kf_conf.carrier_freq_rate_sd_hz_s =
        configuration->property(role + ".carrier_freq_rate_sd_hz_s", kf_conf.carrier_freq_rate_sd_hz_s);
    kf_conf.init_code_phase_sd_chips =
        configuration->property(role + ".init_code_phase_sd_chips", kf_conf.init_code_phase_sd_chips);
    kf_conf.init_carrier_phase_sd_rad =
        configuration->property(role + ".init_carrier_phase_sd_rad", kf_conf.init_carrier_phase_sd_rad);
    kf_conf.init_carrier_freq_sd_hz =
        configuration->property(role + ".init_carrier_freq_sd_hz", kf_conf.init_carrier_freq_sd_hz);
    kf_conf.init_carrier_freq_rate_sd_hz_s =
        configuration->property(role + ".init_carrier_freq_rate_sd_hz_s", kf_conf.init_carrier_freq_rate_sd_hz_s);
}
