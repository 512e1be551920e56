// Job structs and kernel launch entry points of the query-evaluation engine.  The constant blocks the kernels read
// (DevLevel, DevKey, the transform tables and limb maps) are in dev_consts.h.  Layout of all polynomial data is SEAL's
// in-memory order [poly][limb][coeff] of uint64.
#pragma once
#include "launch_ntt.h"
#include "launch_ew.h"
#include "launch_db.h"
#include "launch_roots.h"
#include "launch_behz.h"
#include "launch_mac.h"
// the pure rules host code reads next to the launchers
#include "query_side.h"
#include "bin_merge.h"
#include "bin_rows.h"
#include "bin_eval.h"

// ---- launch wrappers (all asynchronous on `st`), declared per kernel family in the headers above ----
// CONTRACT VOCABULARY of the "contract:" lines in those headers:
//   canonical: a word in [0, m) for the modulus m of its limb (or [0, t) for a plaintext coefficient).
//   RAW:       what an inverse transform leaves where the limb's map entry carries NTT_MAP_RAW -- no twist, no closing reduction; the
//              word w stands for the residue w n^-1 psi^-k mod m at coefficient k.  What the transform can actually leave
//              (ntt_core.h, the last inverse pass, `OUT == IO_GLOBAL && !(INV && RAW)`): for a wide modulus (not ntt_is_narrow) the
//              butterflies keep values in [0, 2^64) by csub_top alone, so ANY 64-bit word; for a narrow modulus, which runs without
//              range control, below (max(2^K b0, 2 b0 + 4 (K - 1)) + 4 (logn - K)) m, with K the stages of the first inverse pass and
//              b0 = 1 for a canonical source or ntt_lazy_bound_q(tab) for the tensor fold's last word (ntt_lazy_input_ok).  The first
//              pass: stage 1 is product-free (2 b0), a later stage doubles a product-free chain and adds 4 m to every other word, so it
//              ends below the larger of 2^K b0 and 2 b0 + 4 (K - 1); every stage of the other passes adds 4 m.  That is under 2^64 by
//              the narrow criterion (b0 = 1: at most 4 logn - 2) or by ntt_lazy_input_ok, and nothing tighter is argued.
//              Every RAW consumer therefore takes ANY 64-bit word: its first operation on
//              the word is a Shoup product (mul_shoup / mul_shoup_lazy, modmath.h: exact for any 64-bit x, m < 2^63).
