#!/bin/sh
# Builds oracle/_ref/libtetra_burst_ref.so (and libtetra_lmac_ref.so, below) from the REFERENCE's own source files, compiled where it lies under
# /root/reference (nothing is copied, no stand-in headers or stubs are written): src/decoder/src/phy/tetra_burst.c
# holds tetra_find_train_seq() (the training-sequence search, :271-341), the burst builders
# build_sync_c_d_burst() / build_norm_c_d_burst() (:171-269) and tetra_burst_rx_cb() (:343-393); phy/tetra_burst_sync.c holds
# the synchroniser state machine tetra_burst_sync_in() (:54-155); tetra_tdma.c its slot counter.  tetra_burst_rx_cb() calls
# tp_sap_udata_ind() of the lower MAC, which stays undefined in the shared object: the checker loads it with lazy binding
# (RTLD_LAZY) after the test-side recorder below.  Output only into oracle/_ref/ (git-ignored; travels to the GPU box with the snapshot).
# No-op when /root/reference is absent (the GPU box uses the prebuilt file).
set -e
REF=${TETRA_REFERENCE_DIR:-/root/reference}
HERE=$(cd "$(dirname "$0")" && pwd)
SRC="$REF/src/decoder/src"
if [ ! -f "$SRC/phy/tetra_burst.c" ]; then
    echo "reference sources not present ($SRC): keeping any prebuilt oracle/_ref"
    exit 0
fi
mkdir -p "$HERE/_ref"
gcc -O2 -std=gnu11 -fPIC -shared -w -I"$SRC" -o "$HERE/_ref/libtetra_burst_ref.so" "$SRC/phy/tetra_burst.c" "$SRC/phy/tetra_burst_sync.c" "$SRC/tetra_tdma.c"
echo "built $HERE/_ref/libtetra_burst_ref.so from $SRC/phy/tetra_burst.c, phy/tetra_burst_sync.c, tetra_tdma.c"
# The one downstream callback of that library, tp_sap_udata_ind, gets a TEST-SIDE recorder (our code, tests/refrec/, compiled
# against the reference's headers; a separate object so that the library above stays reference sources only).  With it the
# reference's own tetra_burst_sync_in() / tetra_burst_rx_cb() run in the tests (tests/test_burst_sync.py).
gcc -O2 -std=gnu11 -fPIC -shared -Wall -I"$SRC" -o "$HERE/_ref/libtetra_tpsap_recorder.so" "$HERE/../tests/refrec/tp_sap_recorder.c"
echo "built $HERE/_ref/libtetra_tpsap_recorder.so (test-side recorder for tp_sap_udata_ind)"
# Lower-MAC channel-coding primitives, again the reference's own files compiled in place:
# scrambler, block (de)interleaver, RCPC (de)puncturer + mother-code encoder, CRC16, and the K=5 rate-1/4 Viterbi decoder
# (viterbi_dec_sb1_wrapper -> conv_cch_decode -> osmo_conv_decode).  tetra_lower_mac.c itself (tp_sap_udata_ind) is not in THIS
# library (it is in libtetra_rxchain_ref.so, below); the checker chains the primitives in the order its lines :181-227 call them
# (oracle/ref_binding.py: lmac_decode).
LM="$SRC/lower_mac"
gcc -O2 -std=gnu11 -fPIC -shared -w -I"$SRC" -o "$HERE/_ref/libtetra_lmac_ref.so" \
    "$LM/tetra_scramb.c" "$LM/tetra_interleave.c" "$LM/tetra_conv_enc.c" "$LM/crc_simple.c" \
    "$LM/viterbi.c" "$LM/viterbi_cch.c" "$LM/osmo_conv.c"
echo "built $HERE/_ref/libtetra_lmac_ref.so from $LM/{tetra_scramb,tetra_interleave,tetra_conv_enc,crc_simple,viterbi,viterbi_cch,osmo_conv}.c"
# The reference's lower MAC itself, tp_sap_udata_ind (lower_mac/tetra_lower_mac.c), behind its own tetra_burst_sync_in / tetra_burst_rx_cb:
# libtetra_rxchain_ref.so.  The reference's files are compiled where they lie; what tetra_lower_mac.c needs from downstream (the upper
# MAC's upper_mac_prim_recv, update_current_network, the ETSI codec's five entry points) is the TEST-SIDE recorder
# tests/refrec/tmv_sap_recorder.c, and the two codec headers it includes are our stand-ins under tests/refrec/standin/c-code/.
# -Wl,-Bsymbolic: the library's tetra_burst_rx_cb calls its OWN tp_sap_udata_ind and uses its OWN t_phy_state, even with the recorder
# above loaded RTLD_GLOBAL in the same process.  Pins the SYNC tracker (tests/test_sync_track.py).
gcc -O2 -std=gnu11 -fPIC -shared -w -I"$SRC" -I"$SRC/lower_mac" -I"$HERE/../tests/refrec/standin" -Wl,-Bsymbolic -Wl,--no-undefined \
    -o "$HERE/_ref/libtetra_rxchain_ref.so" "$HERE/../tests/refrec/tmv_sap_recorder.c" \
    "$LM/tetra_lower_mac.c" "$SRC/tetra_common.c" "$SRC/phy/tetra_burst.c" "$SRC/phy/tetra_burst_sync.c" "$SRC/tetra_tdma.c" \
    "$LM/tetra_scramb.c" "$LM/tetra_interleave.c" "$LM/tetra_conv_enc.c" "$LM/crc_simple.c" \
    "$LM/viterbi.c" "$LM/viterbi_cch.c" "$LM/osmo_conv.c"
echo "built $HERE/_ref/libtetra_rxchain_ref.so from $LM/tetra_lower_mac.c, tetra_common.c, phy/tetra_burst{,_sync}.c, tetra_tdma.c, the lower-MAC primitives + tests/refrec/tmv_sap_recorder.c"
# The reference's per-sample DSP objects (src/dsp/pi4dqpsk, fll, complex_fd, pi4dqpsk_costas, dqpsk_sym_extr, bit_unpacker), again
# compiled where they lie, against OUR stand-in SDR++ core headers (tests/refshim/, see its README.md) and the test-side driver
# tests/refshim/ref_driver.cpp: libref_shim.so with pi spelt as the double constant, libref_shim_fpi.so with the float macro
# (-DREFSHIM_FLOAT_PI).  Loaded by tests/test_reference_shim.py and tests/test_sdrpp_tables.py.
# -ffp-contract=off: the reference's expressions as written (an x86 build never fuses them);
# -fno-access-control: ref_driver.cpp reads the objects' protected / private loop state (ref_get_state).
DSP="$REF/src/dsp"
SHIM="$HERE/../tests/refshim"
shim() {
    g++ -std=c++17 -O2 -ffp-contract=off -fno-access-control -fPIC -shared -w "$@" -I"$SHIM" -I"$REF/src" "$SHIM/ref_driver.cpp" \
        "$DSP/pi4dqpsk.cpp" "$DSP/fll.cpp" "$DSP/complex_fd.cpp" "$DSP/pi4dqpsk_costas.cpp" "$DSP/dqpsk_sym_extr.cpp" "$DSP/bit_unpacker.cpp"
}
if [ -f "$DSP/pi4dqpsk.cpp" ]; then
    shim -o "$HERE/_ref/libref_shim.so" & p0=$!
    shim -DREFSHIM_FLOAT_PI -o "$HERE/_ref/libref_shim_fpi.so" & p1=$!
    wait $p0
    wait $p1
    echo "built $HERE/_ref/libref_shim.so, libref_shim_fpi.so from $DSP/{pi4dqpsk,fll,complex_fd,pi4dqpsk_costas,dqpsk_sym_extr,bit_unpacker}.cpp"
fi
