// Stand-in for <netcdf.h>: included through a common header, no netCDF call is compiled.
#pragma once
