// ref_hydrasdr_wrap.c -- TEST INFRASTRUCTURE: the reference's src/hydrasdr.c, included unmodified where it lies (never copied), so that its
// static rx_callback() -- the per-sample conversion switch that chz_input_write_raw replaces -- can be called on files of raw samples.
// tests/test_raw_input_reference.py builds this as a program in its tmp_path against tests/c/shims/libhydrasdr/hydrasdr.h (declarations only)
// and the reference's airspy-unpack.c; what main() cannot reach of hydrasdr.c (set-up, tuning, the monitor thread) is discarded at link time.
//   ref_hydrasdr <sample type 0..9, hydrasdr.c's Sample_type_name[]> <bits per sample> <isreal 0|1> <scale, %a> <samples> <raw in> <floats out>
// prints "<overranges> <if_power %.17g> <Power_alpha %.17g>": if_power starts at 0, so one callback leaves Power_alpha * energy / samples.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "hydrasdr.c"

// the input half of the fast convolver is not under test: the callback has already stored its floats through input_write_pointer
int write_rfilter(struct filter_in * restrict f, float const * restrict buffer, int size) { (void)f; (void)buffer; (void)size; return 0; }
int write_cfilter(struct filter_in * restrict f, float complex const * restrict buffer, int size) { (void)f; (void)buffer; (void)size; return 0; }
// what the software AGC branch of rx_callback() (off here) can reach
int Verbose = 0;
double scale_ADpower2FS(struct frontend const *frontend) { (void)frontend; return 1.0; }
double scale_AD(struct frontend const *frontend) { (void)frontend; return 1.0; }
int hydrasdr_set_gain(struct hydrasdr_device *device, enum hydrasdr_gain_type type, uint8_t value) { (void)device; (void)type; (void)value; return HYDRASDR_SUCCESS; }
int hydrasdr_get_gain(struct hydrasdr_device *device, enum hydrasdr_gain_type type, hydrasdr_gain_info_t *info) { (void)device; (void)type; info->value = 0; return HYDRASDR_SUCCESS; }
const char *hydrasdr_error_name(int err) { (void)err; return "stub"; }

int main(int argc, char **argv) {
  if (argc != 8) { fprintf(stderr, "usage: ref_hydrasdr type bits isreal scale samples in out\n"); return 2; }
  int const type = atoi(argv[1]), bits = atoi(argv[2]), isreal = atoi(argv[3]), n = atoi(argv[5]);
  double const scale = strtod(argv[4], NULL);
  size_t const in_bytes = (size_t)n * 8 + 64;                    // more than any format takes
  void *raw = NULL;
  if (posix_memalign(&raw, 32, in_bytes) != 0) return 3;
  memset(raw, 0, in_bytes);
  FILE *fi = fopen(argv[6], "rb");
  if (!fi) return 4;
  size_t const got = fread(raw, 1, in_bytes, fi);
  fclose(fi);
  if (got == 0) return 5;
  size_t const nfloat = (size_t)n * (isreal ? 1 : 2);
  float *out = NULL;
  if (posix_memalign((void **)&out, 32, nfloat * sizeof(float) + 64) != 0) return 3;

  struct frontend frontend;
  struct sdrstate sdr;
  memset(&frontend, 0, sizeof frontend);
  memset(&sdr, 0, sizeof sdr);
  sdr.frontend = &frontend;
  frontend.context = &sdr;
  sdr.sample_type = (enum hydrasdr_sample_type)type;
  sdr.scale = scale;
  sdr.software_agc = false;
  frontend.isreal = isreal != 0;
  frontend.bitspersample = bits;
  frontend.samprate = 1e6;
  frontend.if_power = 0;
  if (isreal) frontend.in.input_write_pointer.r = out;
  else frontend.in.input_write_pointer.c = (float complex *)out;
  Name_set = true;                                               // the callback's thread is this program's only one: leave its name alone

  hydrasdr_transfer transfer;
  memset(&transfer, 0, sizeof transfer);
  transfer.ctx = &sdr;
  transfer.samples = raw;
  transfer.sample_count = n;
  if (rx_callback(&transfer) != 0) return 6;

  FILE *fo = fopen(argv[7], "wb");
  if (!fo) return 4;
  if (fwrite(out, sizeof(float), nfloat, fo) != nfloat) return 7;
  fclose(fo);
  printf("%llu %.17g %.17g\n", (unsigned long long)frontend.overranges, frontend.if_power, Power_alpha);
  return 0;
}
