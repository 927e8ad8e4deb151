// The Kalman-loop instances of trk_kernel (trk.hip) in a translation unit of their own.
#define GSDR_TRK_KF_UNIT 1
#include "trk.hip"
