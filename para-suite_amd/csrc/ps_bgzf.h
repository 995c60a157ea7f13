// ps_bgzf.h -- BGZF blocks compressed on the device (ps_bgzf.hip; the encoder of one block is ps_deflate.h).
#pragma once
#include <stdint.h>
#include <string>
#include "ps_bam.h"

namespace ps {

struct BgzfStats { uint32_t n_blocks = 0, n_stored = 0, n_fixed = 0, n_dynamic = 0; uint64_t in_bytes = 0, out_bytes = 0; double kernel_ms = 0; };

// The switch of ps_bgzf_device / PS_BGZF_GPU: device >= 0 registers the device compressor with ps_bam.cpp's batch function
// (every BAM written from then on), -1 takes it out again and gives the device and page-locked buffers back.  Throws when there is no such device.
void bgzf_set_device(int device);

// spans of at most 0xff00 bytes -> comp[k] = the whole BGZF member of spans[k].  One workgroup per block, one launch per round of
// at most PS_BGZF_PIECE input bytes (default 64 MiB, at least one block); PS_BGZF_BTYPE=stored|fixed|dynamic restricts the
// encodings (tests).  Calls are serialised: they share one set of staging and device buffers.
void bgzf_device_compress(const BgzfSpan *spans, size_t n_spans, int device, std::string *comp, BgzfStats *stats);
// The same for a stream that lies on `device` already (the sorted records of ps_bamsort.hip): d_stream[0, n_bytes) cut at 0xff00
// bytes -> comp[k], (n_bytes + 0xff00 - 1) / 0xff00 members.  A round's kernel reads the stream in place: no staging copy, no
// upload; sizes, CRCs and packed images come down as before.  The bytes are the ones bgzf_device_compress makes of the same input.
void bgzf_device_compress_resident(const uint8_t *d_stream, uint64_t n_bytes, int device, std::string *comp, BgzfStats *stats);
int bgzf_device_current();                      // the switch: -1 off

}  // namespace ps
