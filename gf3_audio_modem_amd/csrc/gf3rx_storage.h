// A fp64 value in the context's storage type, as the sample-domain stages write it (gf3rx_blank.hip, gf3rx_resample.hip):
// rint (half to even) clamped to the range for the integer types, a cast for f32.
#pragma once
#include "gf3rx_device.h"

template <int DT> GF3_DEV typename RawT<DT>::E to_storage(double v);
template <> GF3_DEV double to_storage<DT_F64>(double v) { return v; }
template <> GF3_DEV float to_storage<DT_F32>(double v) { return (float)v; }
template <> GF3_DEV int16_t to_storage<DT_I16>(double v) { return (int16_t)fmin(fmax(rint(v), -32768.0), 32767.0); }
template <> GF3_DEV uint8_t to_storage<DT_U8>(double v) { return (uint8_t)fmin(fmax(rint(v), 0.0), 255.0); }
