// Compile coverage of TfheBitExtractT in include/pfhe.hpp, compiled only and never run: the class template instantiated for
// both word types and the alias pair pinned to its C handle types.  tests/test_tfhe_bitext_cpu.py compares the pfhe_*
// symbols this unit leaves undefined with the 306 of cpp_mirror_symbols.txt plus cpp_mirror_bitext_symbols.txt.
#include <type_traits>
#include <utility>

#include "pfhe.hpp"

namespace pfhe {
template class TfheBitExtractT<uint64_t>;
template class TfheBitExtractT<uint32_t>;
}  // namespace pfhe

static_assert(!std::is_same<pfhe::TfheBitExtract, pfhe::TfheBitExtract32>::value, "TfheBitExtract and TfheBitExtract32 are one type");
static_assert(std::is_same<decltype(std::declval<const pfhe::TfheBitExtract &>().handle()), pfhe_bitext *>::value,
              "TfheBitExtract");
static_assert(std::is_same<decltype(std::declval<const pfhe::TfheBitExtract32 &>().handle()), pfhe_bitext32 *>::value,
              "TfheBitExtract32");
static_assert(std::is_move_constructible<pfhe::TfheBitExtract>::value && !std::is_copy_constructible<pfhe::TfheBitExtract>::value &&
                  !std::is_copy_assignable<pfhe::TfheBitExtract32>::value,
              "a handle owner moves and does not copy");

// what the class inherits from its owner is instantiated by use
template <class W>
size_t every_inherited_call(const pfhe::TfheBitExtractT<W> &bx) {
    return bx.in_use() ? 0 : bx.scratch_bytes();
}
template size_t every_inherited_call<uint64_t>(const pfhe::TfheBitExtract &);
template size_t every_inherited_call<uint32_t>(const pfhe::TfheBitExtract32 &);
