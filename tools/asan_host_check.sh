#!/bin/bash
# Host-side AddressSanitizer + UBSan build of the whole library + examples/main.cpp in ONE executable (device code is built
# unsanitised: GPU ASan is not available on this pool), then a micro-model run through every host path main.cpp touches
# (weight load from memory, state arena, encoder + prefill + greedy loop, graph capture / replay, token copy-out, teardown).
#   tools/asan_host_check.sh build      (here: hipcc cross-compiles)
#   tools/asan_host_check.sh run        (on the GPU box)
set -euo pipefail
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
EXE="$ROOT/examples/whisper_main_asan"
CSRC="$ROOT/whisper.mojo_amd/csrc"
PROBE="$ROOT/tools/micro/asan_exit_probe"
SANFLAGS="-Xarch_host -fsanitize=address -Xarch_host -fsanitize=undefined -Xarch_host -fno-omit-frame-pointer"
if [ "${1:-build}" = build ]; then
  # the library's sources as build.py lists them: no copy of the list to fall behind
  SRCS=$(cd "$ROOT/whisper.mojo_amd" && python3 -c 'import sys; sys.path.insert(0, "."); import build; print(" ".join(build.SOURCES))')
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Wall -Wno-unused-function -ffp-contract=on $SANFLAGS \
    -I "$ROOT/include" -x hip $(for s in $SRCS; do echo "$CSRC/$s"; done) \
    -x hip "$ROOT/examples/main.cpp" -o "$EXE"
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O1 -g -std=c++17 $SANFLAGS -x hip "$ROOT/tools/micro/asan_exit_probe.hip" -o "$PROBE"
  echo "built $EXE and $PROBE"
else
  export ASAN_OPTIONS=detect_leaks=0:abort_on_error=0:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1
  # The one report this script may tolerate — and only if a BARE HIP program (tools/micro/asan_exit_probe.hip: no code of this
  # repository) shows it too on this box: the sanitizer's own device allocator CHECK at process exit,
  #   AddressSanitizer: CHECK failed: sanitizer_allocator_device.h:<n> "((!dev_runtime_unloaded_)) != (0)"
  # raised while the sanitizer recycles its quarantine after main has returned ("Done." printed) — from __cxa_finalize ->
  # libamdhip64 -> libhsa-runtime64 -> operator delete, or from an exiting thread's AsanThread::Destroy -> CommitBack: the
  # quarantine then still holds freed DEVICE chunks (under host ASan every hipMalloc is a chunk of the sanitizer's device
  # allocator), and recycling one after the HSA runtime has unloaded trips the CHECK (probe modes 3 / 4 say which pattern does).
  SIG='AddressSanitizer: CHECK failed: sanitizer_allocator_device.h:[0-9]* "((!dev_runtime_unloaded_)) != (0)"'
  probe_sig=0
  for mode in 0 1 2 3 4 5 6; do
    log=$(mktemp); rc=0
    "$PROBE" $mode > "$log" 2>&1 || rc=$?
    if grep -q "$SIG" "$log"; then probe_sig=1; echo "[probe mode $mode] exit $rc: shows the exit-time device-allocator CHECK (bare HIP program)";
    else echo "[probe mode $mode] exit $rc: no sanitizer report"; fi
    grep -q "^Done\.$" "$log" || { echo "probe mode $mode did not finish"; cat "$log"; exit 1; }
    if [ $rc -ne 0 ] && ! grep -q "$SIG" "$log"; then echo "probe mode $mode failed for another reason"; cat "$log"; exit 1; fi
  done
  run() {
    local log rc=0; log=$(mktemp)
    "$EXE" "$@" > "$log" 2>&1 || rc=$?
    cat "$log"
    local bad=0
    grep -q "ERROR: AddressSanitizer\|runtime error:\|SUMMARY: .*Sanitizer" "$log" && bad=1
    grep -q "^Done\.$" "$log" || bad=1
    if grep -q "AddressSanitizer: CHECK failed" "$log"; then
      # tolerated only as the probe's signature, once, after "Done.", with __cxa_finalize and no frame of this executable's own code above it
      if [ $probe_sig -eq 1 ] && [ "$(grep -c 'AddressSanitizer: CHECK failed' "$log")" = 1 ] && grep -q "$SIG" "$log" && \
         [ "$(grep -n '^Done\.$' "$log" | cut -d: -f1)" -lt "$(grep -n 'CHECK failed' "$log" | cut -d: -f1)" ] && \
         grep -q "Quarantine.*Recycle" "$log" && grep -q "__cxa_finalize\|AsanThread::Destroy" "$log" && \
         ! grep -q "whisper_mi\.cpp\|wm_[a-z]*\.cpp\|kernels_.*\.hip\|main\.cpp" "$log"; then
        echo "[tolerated] exit-time device-allocator CHECK of the sanitizer runtime (the bare probe shows it too); exit code $rc"
      else
        bad=1
      fi
    elif [ $rc -ne 0 ]; then
      bad=1  # a non-zero exit without that signature is a failure
    fi
    if [ $bad -ne 0 ]; then echo "ASAN/UBSAN host check: FAILED ($*) exit $rc"; exit 1; fi
  }
  for dt in f32 bf16; do
    run --config micro --synthetic-weights 0 --synthetic-mel 1000 --dtype $dt --prompt 1,2,3,4 --eot 532 --max-loop 40 --vocab /nonexistent
  done
  # the pipelined entry under the sanitizer: coalesced pairs (a held submit, pair states, row demultiplexing) and the library's
  # pump thread feeding natural-stop loops in sub-chunks (max-loop 40 > two sub-chunks) — 13 submits: six pairs and a leftover
  run --config micro --synthetic-weights 0 --synthetic-mel 1000 --dtype f32 --prompt 1,2,3,4 --eot 999999 --max-loop 40 --vocab /nonexistent --pipelined 13
  run --config micro --synthetic-weights 0 --synthetic-mel 1000 --dtype bf16 --prompt 1,2,3,4 --eot 532 --max-loop 40 --vocab /nonexistent --pipelined 5
  # Whisper-tiny in bf16: the encoder's row-panel / full-row GEMM launchers and the fused LayerNorm plumbing (d = 384 only)
  run --config tiny --synthetic-weights 0 --synthetic-mel 1000 --dtype bf16 --max-loop 6 --vocab /nonexistent
  echo "ASAN/UBSAN host check: clean"
fi
