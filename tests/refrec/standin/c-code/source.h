/* Stand-in for the ETSI TETRA speech codec's source-coding header (see channel.h beside it): our own prototypes for the three
 * functions lower_mac/tetra_lower_mac.c calls on a traffic slot; defined, aborting, by tests/refrec/tmv_sap_recorder.c. */
#ifndef REFREC_STANDIN_SOURCE_H
#define REFREC_STANDIN_SOURCE_H
#include <stdint.h>
void Bits2prm_Tetra(int16_t serial[], int16_t parm[]);
void Decod_Tetra(int16_t parm[], int16_t synth[]);
void Post_Process(int16_t synth[], int16_t length);
#endif
