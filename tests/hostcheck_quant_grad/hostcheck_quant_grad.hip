// hostcheck_quant_grad.hip -- TEST SHIM: runs quant_math.h's quant_grad_slot -- the slot -> (book, id byte, gradient element)
// mapping the kernel of r3dgs_quantised_codebook_grad executes per lane -- on the CPU, with the decoder's ragged-offset
// arithmetic in front of it exactly as in the kernel, so tests/test_quantised_grad_cpu.py can hold the enumeration to a
// numpy restatement WITHOUT a GPU.  Not part of the product; nothing in reduced-3dgs_amd/ links it.
#include "../../reduced-3dgs_amd/csrc/quant_math.h"

extern "C" {

int hqg_slots() { return r3::kQuantSlots; }
int hqg_chunk() { return r3::kQuantGradChunk; }
int hqg_max_groups() { return r3::kQuantGradMaxGroups; }
int hqg_groups(int P) { return r3::quant_grad_groups(P); }
int hqg_chunks_per_group(int P) { return r3::quant_grad_chunks_per_group(P); }

// Every owned slot of every Gaussian, in (Gaussian, slot) order: book, the id byte's value, which tensor, which element, and
// where the id byte sits (id_at >= 0: that byte of sh_ids; < 0: byte -(id_at + 1) of geom_ids).  Room for P * hqg_slots()
// entries; returns how many were written.
long long hqg_enumerate(int P, const int* coeffs, const int* perband, const int* cumsum, const uint8_t* geom_ids,
                        const uint8_t* sh_ids, int* book, int* id, int* tensor, long long* elem, long long* id_at)
{
    long long n = 0;
    for (long long i = 0; i < P; i++) {
        int deg;
        const long long sh_off = 3LL * r3::quant_ragged_offset((int)i, coeffs, perband, cumsum, &deg);
        for (int s = 0; s < r3::kQuantSlots; s++) {
            r3::QuantGradSlot slot;
            if (!r3::quant_grad_slot(s, i, deg, sh_off, geom_ids, sh_ids, &slot)) continue;
            book[n] = slot.book;
            id[n] = *slot.id;
            tensor[n] = slot.tensor;
            elem[n] = slot.elem;
            id_at[n] = s < r3::kQuantGeomSlots ? -(long long)(slot.id - geom_ids) - 1 : (long long)(slot.id - sh_ids);
            n++;
        }
    }
    return n;
}

}  // extern "C"
