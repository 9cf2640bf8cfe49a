/* mrcal_amd: the anti-aliasing Gaussian pre-filter is declared in mrcal_amd.h ("smoothing"), with everything else.
   This header is kept for the callers that include it by name */
#pragma once
#include "mrcal_amd.h"
