// azk_search.hip - the translation unit of the three engine families that search or judge a position: azk_tree.hip (the AlphaZero
// step), azk_vanilla.hip (vanilla MCTS) and azk_rules.hip (stateless rules, row softmax).  They are ONE unit, in this order, because
// they share the device functions of azk_device.h that are not force-inlined - azk_valid_moves_gomoku and azk_pairwise_sum - and the
// compiler shapes such a function by ALL its callers in the unit before it inlines it: compiled apart, k_vanilla (5 470 -> 5 544
// instructions), k_rules and k_softmax_rows (709 -> 708) come out with other instruction streams, and k_tree<false, true, false,
// false, 4> with one other instruction.  Each part compiles on its own too (tools/kernel_resources.sh); the other engine files
// share only force-inlined functions and are units of their own.
#include "azk_tree.hip"
#include "azk_vanilla.hip"
#include "azk_rules.hip"
