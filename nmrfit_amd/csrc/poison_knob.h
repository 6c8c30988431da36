// poison_knob.h -- how the diagnostic NMRFIT_POISON_ALLOC is read (host_call.hip, device_alloc): a decimal byte value
// 0..255 fills every new device block with that byte; unset, empty, or anything else -- a sign, a fraction, trailing
// text, a value above 255 -- leaves the knob off.  Plain C++ with no HIP in it, so that a host program can test it.
#pragma once

namespace nmrfit {

// the byte to fill with, or -1: no fill
inline int parse_poison_byte(const char *text)
{
    if (!text || !*text) return -1;
    int v = 0, digits = 0;
    for (const char *c = text; *c; ++c) {
        if (*c < '0' || *c > '9' || ++digits > 3) return -1;
        v = 10 * v + (*c - '0');
    }
    return v <= 255 ? v : -1;
}

}  // namespace nmrfit
