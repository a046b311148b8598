/* Linked with sufr_amd/csrc/sufr_host_stubs.cpp alone (the device side of the ABI as "no device" stubs): the limit of the
 * listed-byte retry and its two getters answer as every stubbed entry point does. */
#include <stdio.h>
#include <string.h>

#include "sufr_hip.h"

int main(void)
{
    int bad = 0;
    sufr_hip_ctx *ctx = sufr_hip_create(0);
    if (ctx != NULL) { fprintf(stderr, "the stubs created a context\n"); bad = 1; }
    if (sufr_hip_set_exc_max_affected(NULL, 5) != SUFR_HIP_E_NO_DEVICE) { fprintf(stderr, "set_exc_max_affected(5) = %d\n", sufr_hip_set_exc_max_affected(NULL, 5)); bad = 1; }
    if (sufr_hip_set_exc_max_affected(NULL, 0) != SUFR_HIP_E_NO_DEVICE) { fprintf(stderr, "set_exc_max_affected(0) is not the no-device code\n"); bad = 1; }
    if (sufr_hip_set_exc_max_affected(NULL, ((uint64_t)1 << 22) + 1) != SUFR_HIP_E_NO_DEVICE) { fprintf(stderr, "set_exc_max_affected(2^22 + 1) is not the no-device code\n"); bad = 1; }
    if (sufr_hip_exc_retry(NULL) != 0) { fprintf(stderr, "exc_retry = %d\n", sufr_hip_exc_retry(NULL)); bad = 1; }
    if (sufr_hip_exc_taken(NULL) != 0) { fprintf(stderr, "exc_taken != 0\n"); bad = 1; }
    if (strstr(sufr_hip_last_error(NULL), "no HIP device") == NULL) { fprintf(stderr, "last_error: %s\n", sufr_hip_last_error(NULL)); bad = 1; }
    if (!bad) printf("stubs: no device %d, exc_retry 0, exc_taken 0\n", SUFR_HIP_E_NO_DEVICE);
    return bad;
}
