/* tests/c/shims/libhydrasdr/hydrasdr.h -- TEST INFRASTRUCTURE.  A declarations-only stand-in for the vendor's <libhydrasdr/hydrasdr.h>, written
 * from the names the reference's src/hydrasdr.c uses and from how it uses them, so that tests/c/ref_hydrasdr_wrap.c can compile that file
 * where no HydraSDR library is installed.  Nothing here is the vendor's header: the numbering of the sample types follows hydrasdr.c's own
 * Sample_type_name[] table, every other value is arbitrary; no function declared here is ever defined except by the wrapper's empty stubs. */
#ifndef CHZ_TEST_HYDRASDR_SHIM_H
#define CHZ_TEST_HYDRASDR_SHIM_H
#include <stdbool.h>
#include <stdint.h>

#define HYDRASDR_SUCCESS 0
#define HYDRASDR_VER_MAJOR 1
#define HYDRASDR_VER_MINOR 1
#define HYDRASDR_VER_REVISION 0
#define HYDRASDR_MAKE_VERSION(major, minor, revision) (((uint32_t)(major) << 16) | ((uint32_t)(minor) << 8) | (uint32_t)(revision))

enum hydrasdr_sample_type {
  HYDRASDR_SAMPLE_FLOAT32_IQ = 0, HYDRASDR_SAMPLE_FLOAT32_REAL, HYDRASDR_SAMPLE_INT16_IQ, HYDRASDR_SAMPLE_INT16_REAL, HYDRASDR_SAMPLE_UINT16_REAL,
  HYDRASDR_SAMPLE_RAW, HYDRASDR_SAMPLE_INT8_IQ, HYDRASDR_SAMPLE_UINT8_IQ, HYDRASDR_SAMPLE_INT8_REAL, HYDRASDR_SAMPLE_UINT8_REAL
};
enum hydrasdr_gain_type {
  HYDRASDR_GAIN_TYPE_LNA = 0, HYDRASDR_GAIN_TYPE_RF, HYDRASDR_GAIN_TYPE_MIXER, HYDRASDR_GAIN_TYPE_FILTER, HYDRASDR_GAIN_TYPE_VGA,
  HYDRASDR_GAIN_TYPE_LINEARITY, HYDRASDR_GAIN_TYPE_SENSITIVITY, HYDRASDR_GAIN_TYPE_LNA_AGC, HYDRASDR_GAIN_TYPE_RF_AGC, HYDRASDR_GAIN_TYPE_MIXER_AGC,
  HYDRASDR_GAIN_TYPE_FILTER_AGC
};
#define HYDRASDR_CAP_LNA_AGC          (1u << 0)
#define HYDRASDR_CAP_RF_AGC           (1u << 1)
#define HYDRASDR_CAP_MIXER_AGC        (1u << 2)
#define HYDRASDR_CAP_FILTER_AGC       (1u << 3)
#define HYDRASDR_CAP_BIAS_TEE         (1u << 4)
#define HYDRASDR_CAP_PACKING          (1u << 5)
#define HYDRASDR_CAP_LINEARITY_GAIN   (1u << 6)
#define HYDRASDR_CAP_SENSITIVITY_GAIN (1u << 7)
#define HYDRASDR_CAP_LNA_GAIN         (1u << 8)
#define HYDRASDR_CAP_RF_GAIN          (1u << 9)
#define HYDRASDR_CAP_MIXER_GAIN       (1u << 10)
#define HYDRASDR_CAP_FILTER_GAIN      (1u << 11)
#define HYDRASDR_CAP_VGA_GAIN         (1u << 12)

struct hydrasdr_device;
typedef struct { uint32_t major_version, minor_version, revision; } hydrasdr_lib_version_t;
typedef struct { int min_value, max_value, default_value; } hydrasdr_gain_range_t;
typedef struct { int value; } hydrasdr_gain_info_t;
typedef struct {
  char board_name[64], firmware_version[128];
  uint32_t features, sample_types, current_adc_bits;
  hydrasdr_gain_range_t linearity_gain, sensitivity_gain, lna_gain, rf_gain, mixer_gain, filter_gain, vga_gain;
  uint32_t current_samplerate, current_hw_samplerate, current_decimation_factor, current_decimation_mode, current_bandwidth, bandwidth_auto_selected,
           current_sample_type, current_packing;
} hydrasdr_device_info_t;
typedef struct {
  struct hydrasdr_device *device;
  void *ctx;
  void *samples;
  int sample_count;
  uint64_t dropped_samples;
  enum hydrasdr_sample_type sample_type;
} hydrasdr_transfer;
typedef int (*hydrasdr_sample_block_cb_fn)(hydrasdr_transfer *transfer);

void hydrasdr_lib_version(hydrasdr_lib_version_t *v);
int hydrasdr_list_devices(uint64_t *serials, int count);
int hydrasdr_open_sn(struct hydrasdr_device **device, uint64_t serial);
int hydrasdr_open(struct hydrasdr_device **device);
int hydrasdr_close(struct hydrasdr_device *device);
const char *hydrasdr_error_name(int err);
int hydrasdr_get_device_info(struct hydrasdr_device *device, hydrasdr_device_info_t *info);
int hydrasdr_set_packing(struct hydrasdr_device *device, uint8_t on);
int hydrasdr_set_sample_type(struct hydrasdr_device *device, enum hydrasdr_sample_type type);
int hydrasdr_get_samplerates(struct hydrasdr_device *device, uint32_t *rates, uint32_t count);
int hydrasdr_set_samplerate(struct hydrasdr_device *device, uint32_t rate);
int hydrasdr_set_gain(struct hydrasdr_device *device, enum hydrasdr_gain_type type, uint8_t value);
int hydrasdr_get_gain(struct hydrasdr_device *device, enum hydrasdr_gain_type type, hydrasdr_gain_info_t *info);
int hydrasdr_set_rf_bias(struct hydrasdr_device *device, uint8_t on);
int hydrasdr_set_freq(struct hydrasdr_device *device, uint64_t hz);
int hydrasdr_start_rx(struct hydrasdr_device *device, hydrasdr_sample_block_cb_fn cb, void *ctx);
int hydrasdr_stop_rx(struct hydrasdr_device *device);
int hydrasdr_is_streaming(struct hydrasdr_device *device);
#endif
