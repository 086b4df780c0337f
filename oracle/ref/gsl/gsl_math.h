/* stand-in for <gsl/gsl_math.h>: everything lives in gsl_standin.h (TEST INFRASTRUCTURE ONLY) */
#include "gsl_standin.h"
