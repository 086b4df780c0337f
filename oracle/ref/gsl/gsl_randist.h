/* stand-in for <gsl/gsl_randist.h>: everything lives in gsl_standin.h (TEST INFRASTRUCTURE ONLY) */
#include "gsl_standin.h"
