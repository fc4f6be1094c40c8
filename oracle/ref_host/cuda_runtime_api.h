// Stand-in (the project's own text, see ref_host.hpp): the reference includes <cuda_runtime_api.h>.
#pragma once
#include "ref_host.hpp"
