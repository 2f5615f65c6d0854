// Head dimension and staged tile height shared by the attention backward
// kernels (fa_bwd_prep.hip, fa_bwd_v3.hip, fa_bwd_dq_v5.hip,
// fa_bwd_dkv_v6.hip); the fragment types and conversions are fa_tile.h's.
#pragma once
#include "fa_tile.h"

#define FB3_D 128
#define FB3_QT 64           // q rows per staged tile (2 sub-tiles of 32)
