// C ABI of the host JPEG entropy decoder (jpeg_host.h): no HIP call, no global state.
#include <stdint.h>

#include "jpeg_host.h"
#include "sdpnet_hip.h"

extern "C" int sdp_jpeg_probe(const uint8_t* data, int64_t len, int32_t* info) {
  return sdpjpeg::probe(data, len, info);
}

extern "C" int sdp_jpeg_entropy_decode(const uint8_t* data, int64_t len, int16_t* coef, int64_t coef_cap,
                                       uint8_t* qt, int32_t* info) {
  return sdpjpeg::entropy_decode(data, len, coef, coef_cap, qt, info);
}
