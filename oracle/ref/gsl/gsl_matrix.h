/* stand-in for <gsl/gsl_matrix.h>: everything lives in gsl_standin.h (TEST INFRASTRUCTURE ONLY) */
#include "gsl_standin.h"
