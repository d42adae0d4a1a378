#!/bin/bash
# tools/scope_series_ab.sh — is k_scope<LOGW, false> (the scope's kernel without a reading series) the parent commit's k_scope<LOGW>,
# instruction for instruction, for the seven windows?  No GPU needed.  First: tools/build_ab.sh (the parent's objects -> lib_ab/obj),
# and the Makefile's build of this tree.  Exit status 0: all seven identical.
top=$(cd "$(dirname "$0")/.." && pwd)
rc=0
for logw in 8 9 10 11 12 13 14; do
	python3 "$top/tools/code_object_ab.py" \
	    "$top/meters.lv2_amd/lib_ab/obj/mtr_scope.o" "_ZN12_GLOBAL__N_17k_scopeILi${logw}EEEv14mtr_scope_args" \
	    "$top/meters.lv2_amd/lib/obj/mtr_scope.o" "_ZN12_GLOBAL__N_17k_scopeILi${logw}ELb0EEEvNSt11conditionalIXT0_E21mtr_scope_series_args14mtr_scope_argsE4typeE" || rc=1
done
exit $rc
