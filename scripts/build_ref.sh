#!/bin/bash
# A/B build of the engine as of a git ref -> scripts/_bin/libfe_<name>.so.  usage: scripts/build_ref.sh <name> <git-ref> [-D...]
# (the ref's own sources and, where it has one, its own build recipe: a ref from before the engine was two units builds its single file)
NAME=$1; REF=$2; shift 2
D=/tmp/fe_ref_$NAME; rm -rf $D; mkdir -p $D
cd "$(dirname "$0")/.." && git archive $REF fluidlab_amd/csrc include __graft_entry__.py | tar -x -C $D && SRC=$D scripts/build_variant.sh $NAME "$@"
