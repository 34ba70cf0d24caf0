cd /tmp && export TMPDIR=/tmp; cd $GRAFT_REPO_ROOT
# usage: [OUT=dir] bash tools/prof_chain_round.sh      (writes $OUT/r05_*, default profile_out/)
OUT=${OUT:-profile_out}
mkdir -p $OUT
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/p_trace -o r -- python bench.py --full --no-cpu-baseline --no-decode --no-ragged --no-extra --steps 4 --warmup 3 > /dev/null 2>&1
python tools/prof_chain.py $OUT/p_trace > $OUT/r05_chain.txt 2>&1
python tools/prof_phases.py $OUT/p_trace > $OUT/r05b_step_phases.txt 2>&1
rm -rf $OUT/p_trace
rocprofv3 --kernel-trace --output-format csv -d $OUT/p_g -o g -- python tools/prof_greedy.py run > /dev/null 2>&1
python tools/prof_greedy.py $OUT/p_g > $OUT/r05_greedy_bs1_nodes.txt 2>&1
rm -rf $OUT/p_g
