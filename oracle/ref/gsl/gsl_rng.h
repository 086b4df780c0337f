/* stand-in for <gsl/gsl_rng.h>: everything lives in gsl_standin.h (TEST INFRASTRUCTURE ONLY) */
#include "gsl_standin.h"
