/* TEST-ONLY: lets tests/cpp/ref_pres_shim.cpp parse the reference headers that include <netcdf.h> (include/netcdf_interface.h).
 * The one macro those headers name and nothing else: no type, no function. */
#ifndef MHH_TEST_NETCDF_STUB
#define MHH_TEST_NETCDF_STUB
#define NC_UNLIMITED 0L
#endif
