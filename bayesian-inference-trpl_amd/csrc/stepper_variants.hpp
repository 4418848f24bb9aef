// THE list of stepper launchers: one TRPL_VARIANT(sink, predict, unit) line per launcher that exists.  No include guard: the
// reader defines TRPL_VARIANT and includes this file (trpl_common.hpp declares the launchers from it, trpl_api.hip fills its
// table from it); the Makefile reads the same lines for the objects to build.  A line's object is
// stepper_[<sink>_][predict_]<unit>.o ("plain" and predict 0 leave no word).  The units fast, strict, pair, f32, mixed and hist32
// at (plain, 0) have a source file of their own; every other line is one more compilation of stepper_variant.hip (fast, strict)
// or stepper_pair_variant.hip (pair), with -DTRPL_STEPPER_<WORD>=1 for each of its words.  Keep one line per variant, in this form.
//   sink:    plain | moments (TRPL_FLAG_MOMENTS) | weighted (TRPL_FLAG_WEIGHTED) | cut (TRPL_FLAG_CUT; batched sink: no strict unit)
//   predict: 1 = TRPL_FLAG_PREDICT
//   unit:    which arithmetic and kernel family, hence which -ffp-contract (Makefile): strict is off, the others on
TRPL_VARIANT(plain, 0, fast)
TRPL_VARIANT(plain, 0, strict)
TRPL_VARIANT(plain, 0, pair)
TRPL_VARIANT(plain, 0, f32)
TRPL_VARIANT(plain, 1, fast)
TRPL_VARIANT(plain, 1, strict)
TRPL_VARIANT(plain, 1, pair)
TRPL_VARIANT(moments, 0, fast)
TRPL_VARIANT(moments, 0, strict)
TRPL_VARIANT(moments, 0, pair)
TRPL_VARIANT(moments, 1, fast)
TRPL_VARIANT(moments, 1, strict)
TRPL_VARIANT(moments, 1, pair)
TRPL_VARIANT(weighted, 0, fast)
TRPL_VARIANT(weighted, 0, strict)
TRPL_VARIANT(weighted, 0, pair)
TRPL_VARIANT(weighted, 1, fast)
TRPL_VARIANT(weighted, 1, strict)
TRPL_VARIANT(weighted, 1, pair)
TRPL_VARIANT(cut, 0, fast)
TRPL_VARIANT(cut, 0, pair)
TRPL_VARIANT(cut, 1, fast)
TRPL_VARIANT(cut, 1, pair)
#ifdef TRPL_EXPERIMENTAL                     // `make EXPERIMENTAL=1` only: the default library must not reference them
TRPL_VARIANT(plain, 0, mixed)
TRPL_VARIANT(plain, 0, hist32)
#endif
