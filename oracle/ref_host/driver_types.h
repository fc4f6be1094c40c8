// Stand-in (the project's own text, see ref_host.hpp): the reference includes <driver_types.h>.
#pragma once
#include "ref_host.hpp"
