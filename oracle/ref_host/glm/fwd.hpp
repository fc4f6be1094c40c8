// Stand-in (the project's own text, not glm's: see glm/glm.hpp): the reference includes <glm/fwd.hpp>.
#pragma once
#include "glm.hpp"
