// Include name of the OpenCV double (oracle/ref_cv/opencv2/core/core.hpp holds all of it).
#include "opencv2/core/core.hpp"
