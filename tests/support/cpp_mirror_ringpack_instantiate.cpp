// Compile coverage of TfheRingPackT in include/pfhe.hpp, compiled only and never run: the class template instantiated for
// both word types and the alias pair pinned to its C handle types.  tests/test_tfhe_ring_pack_cpu.py compares the pfhe_*
// symbols this unit leaves undefined with the 306 of cpp_mirror_symbols.txt plus cpp_mirror_ringpack_symbols.txt.
#include <type_traits>
#include <utility>

#include "pfhe.hpp"

namespace pfhe {
template class TfheRingPackT<uint64_t>;
template class TfheRingPackT<uint32_t>;
}  // namespace pfhe

static_assert(!std::is_same<pfhe::TfheRingPack, pfhe::TfheRingPack32>::value, "TfheRingPack and TfheRingPack32 are one type");
static_assert(std::is_same<decltype(std::declval<const pfhe::TfheRingPack &>().handle()), pfhe_ringpack *>::value,
              "TfheRingPack");
static_assert(std::is_same<decltype(std::declval<const pfhe::TfheRingPack32 &>().handle()), pfhe_ringpack32 *>::value,
              "TfheRingPack32");
static_assert(std::is_move_constructible<pfhe::TfheRingPack>::value && !std::is_copy_constructible<pfhe::TfheRingPack>::value &&
                  !std::is_copy_assignable<pfhe::TfheRingPack32>::value,
              "a handle owner moves and does not copy");

// what the class inherits from its owner is instantiated by use
template <class W>
size_t every_inherited_call(const pfhe::TfheRingPackT<W> &rp) {
    return rp.in_use() ? rp.slot(1, 2) : rp.scratch_bytes();
}
template size_t every_inherited_call<uint64_t>(const pfhe::TfheRingPack &);
template size_t every_inherited_call<uint32_t>(const pfhe::TfheRingPack32 &);
