// The device half of a stream (csrc/device_stream.hpp) for the host-only
// sanitizer build: host_stream.cpp links against these, and a packer-only
// stream (no context) never reaches one that does anything.
#include "../../jepsen-etcd-demo_amd/csrc/common.hpp"
#include "../../jepsen-etcd-demo_amd/csrc/device_stream.hpp"

namespace lcst {
static int none() { return lc::fail(LC_E_DEVICE, "sanitizer build: no device half"); }
int stream_dev_open(lc_ctx *, bool, StreamDev **) { return none(); }
void stream_dev_close(StreamDev *) {}
int stream_dev_max_final(const StreamDev *) { return 0; }
int stream_dev_push(StreamDev *, int64_t, const Item *, int64_t, const uint16_t *, uint64_t, const uint32_t *, uint64_t,
                    uint32_t, std::vector<Dead> *, const SetWork *, std::vector<Final> *) { return none(); }
int stream_dev_peaks(StreamDev *, int64_t, uint32_t *) { return none(); }
int stream_dev_finals(StreamDev *, int64_t, const int32_t *, int64_t, uint32_t, uint64_t *, uint32_t *) { return none(); }
double stream_dev_final_ms(const StreamDev *) { return 0; }
int stream_dev_set_alloc(StreamDev *, int32_t *) { return none(); }
void stream_dev_set_free(StreamDev *, int32_t) {}
int stream_dev_set_record(StreamDev *, int32_t, int64_t, uint32_t *, int64_t) { return none(); }
void stream_dev_set_stats(const StreamDev *, double *) {}
int stream_dev_record(StreamDev *, int64_t, uint32_t *) { return none(); }
void stream_dev_timing(const StreamDev *, double *) {}
}  // namespace lcst

// lc_stream_finish checks deferred keys through the batch path: only with a context.
extern "C" int lc_check_batch(lc_ctx *, const lc_batch *, lc_result *, lc_stats *) { return lcst::none(); }
