/* Stand-in for the ETSI TETRA speech codec's channel-coding header, which the reference's lower MAC includes but which is not part
 * of the reference tree.  Our own prototypes (nothing copied), written from the two call sites in lower_mac/tetra_lower_mac.c; the
 * functions themselves are defined by tests/refrec/tmv_sap_recorder.c and abort: only a traffic slot reaches them. */
#ifndef REFREC_STANDIN_CHANNEL_H
#define REFREC_STANDIN_CHANNEL_H
#include <stdint.h>
int16_t Desinterleaving_Speech(int16_t interleaved[], int16_t coded[]);
int16_t Channel_Decoding(int16_t first_pass, int16_t frame_stealing, int16_t coded[], int16_t reordered[]);
#endif
