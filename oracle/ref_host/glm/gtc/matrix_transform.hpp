// Stand-in (the project's own text, not glm's: see glm/glm.hpp): the reference includes <glm/gtc/matrix_transform.hpp>
// and uses nothing of it.
#pragma once
#include "../glm.hpp"
