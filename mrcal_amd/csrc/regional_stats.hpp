// regional_stats.hip for the other units: the statistics of one camera where they are, on the device
#pragma once
#include "../../include/mrcal_amd.h"

namespace mrcal_amd {
// camera icam's grid and its mean / stdev / count [gridn_height][gridn_width] on the device (complete when _create()
// returned: any stream may read them). Any of the outputs may be NULL. false: set_error() says why
bool regional_statistics_device(const mrcal_amd_regional_statistics_t* s, int icam, int* gridn_width, int* gridn_height,
                                const double** d_mean, const double** d_stdev, const int** d_count);
}
