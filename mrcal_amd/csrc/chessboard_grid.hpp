// Part e of "chessboard corners" (include/mrcal_amd.h): the complete board_width x board_height lattice among N
// refined corner candidates, on the host. No HIP type or call: it works without a GPU, and
// tests/hostcheck/chessboard_grid_check.cpp runs it under the host sanitizers.
#pragma once
#include <stdint.h>

namespace mrcal_amd {

// q (N,2): the candidates; response (N,) or NULL: seeds are tried in descending response (NULL: in the order given);
// status (N,) or NULL: only candidates of status 0 (and finite coordinates) are looked at. true: the board was found and
// corners (board_height, board_width, 2) holds it in the order of the definition. false: no board; corners is untouched
bool chessboard_grid(int N, const double* q, const int32_t* response, const int32_t* status,
                     int board_width, int board_height, double* corners);

} // namespace mrcal_amd
