/* sgm_image_io.h -- minimal image I/O for the command-line driver (sgm_main.c).
 * Grey conversion of colour input follows stb_image's req_comp=1 path, the one the reference's main.c uses
 * (stb_image.h:1746-1749): y = (77 r + 150 g + 29 b) >> 8. */
#ifndef SGM_IMAGE_IO_H
#define SGM_IMAGE_IO_H
#include <stdint.h>

/* Loads PGM (P5), PPM (P6) or PNG (8-bit, non-interlaced; grey, grey+alpha, RGB, RGBA, palette) as 8-bit grey.
 * Returns a malloc'ed buffer of w*h bytes or NULL (message on stderr). */
uint8_t* sgm_load_gray(const char* path, int* w, int* h);

/* Loads a grey image of up to 16 bits per sample as w*h uint16_t samples (malloc'ed; NULL and a message on stderr otherwise):
 * binary PGM (P5) with maxval 256..65535, two bytes per sample, most significant first; PNG grey of depth 16 (*maxval = 65535);
 * and everything sgm_load_gray reads, as the same values unshifted (*maxval = 255). */
uint16_t* sgm_load_gray16(const char* path, int* w, int* h, int* maxval);

/* 8-bit grey writers; return 0 on success. */
int sgm_write_png_gray(const char* path, const uint8_t* data, int w, int h);
int sgm_write_pgm(const char* path, const uint8_t* data, int w, int h);
/* 16-bit binary PGM (maxval 65535, most significant byte first); 0 on success */
int sgm_write_pgm16(const char* path, const uint16_t* data, int w, int h);
#endif
