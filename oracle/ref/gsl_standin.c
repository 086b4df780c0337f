/* oracle/ref/gsl_standin.c -- TEST INFRASTRUCTURE ONLY: the one definition of the stand-in's generator
   functions and shared state (gsl/gsl_standin.h), linked into _ref/mcmc_ref and _ref/ref_driver. */
#define GSL_STANDIN_IMPLEMENTATION
#include "gsl/gsl_standin.h"
